// C ABI of a run-time MODP group (include/mpvss_hip.h, "MODP groups of a run-time modulus"): the group handle, its
// host-side constants and hash_to_scalar, and the batched entry points over modp_rt_kernels.hip.  Included at the end
// of mpvss_capi.cpp (it uses the context, staging and transcript helpers defined there; the transcript is framed by
// frame_update / frame_shares / frame_min_bytes_update at the handle's element size).
//
// Every entry point that touches the device has the same shape: the argument check with its error strings, one RtCall
// (below) for the device, the constants, the chunk loop, the choice of space, the copies back and the wiping of secrets,
// and in between only what is its own -- which buffers its arrays use, which of them are secret, what it launches and
// what it hashes.  The launch decisions (rt_comb_for, rt_dleq_dev, rt_commit_eval_dev with rt_fd_prepare and
// rt_fd_positions_ok, rt_twin_dev, rt_fixed_base_dev, rt_scalar_on_device, rt_share_hash_on_device, rt_product_tree, the grouping of small boxes in
// mpvss_modp_group_verify_many and that of secrets in mpvss_modp_group_reconstruct_many) are single places of their own.

constexpr size_t RT_EB_MAX = FRAME_EB_MAX;     // the widest element / scalar of a handle (mpvss_modp_group_create_wide): 512 bytes

// q, q - 1 and (q-1)/2 for the host-side scalar ring (host_scalar.h) at NW 64-bit words
template <int NW_>
struct RtRings {
  static constexpr int NW = NW_;
  hsc::ModulusRtN<NW_> mod, ord, sub;
};

struct mpvss_modp_group {
  modp_rt_consts c;          // device image of the constants (copied to the device by every call)
  modp_rt_consts cq;         // the same for the modulus q' = (q-1)/2 at the handle's own lpl (R > 4 q' wherever R > 4 q): the scalar
                             // ring Z/(q-1) = Z/2 x Z/q' on the device.  Built only when q' is odd and >= 3 (has_q)
  bool has_q = false;
  bool has_sh = false;       // (q-1)/2 >= 2^256, i.e. bits >= 258: hash_to_scalar is the identity on a SHA-256 output, so the per-share
                             // DLEQ hash may run on the device (k_rt_share_verdict does not reduce)
  uint8_t subR_be[RT_EB_MAX];// R mod q' = 2^(29 L) mod q', eb bytes big-endian (has_q): takes a coefficient into Montgomery form
  uint8_t subm2_be[RT_EB_MAX];// q' - 2, eb bytes big-endian (has_q): Fermat's exponent of an inverse mod q' (rt_lagrange_dev)
  int bits = 0;
  int lpl = 0;
  size_t eb = 0;             // bytes of every element, scalar and exponent of this handle on the ABI: 256, 384 or 512
  uint8_t sub_be[RT_EB_MAX]; // (q-1)/2 big-endian, eb bytes: hash_to_scalar's modulus (modp.rs:142-148)
  uint8_t g_be[RT_EB_MAX];   // subgroup generator 4 (modp.rs:65-66 for any q >= 5)
  uint8_t G_be[RT_EB_MAX];   // main generator 2
  uint8_t q_be[RT_EB_MAX];
  RtRings<32> r32;           // the rings of a 256-byte handle ...
  RtRings<48> r48;           // ... of a 384-byte one ...
  RtRings<64> r64;           // ... and of a 512-byte one (the other two stay unset)
};

// A key set of a run-time group (include/mpvss_hip.h, "Key sets of a run-time group"): the rows of n public keys on the device
// (modp_rt_launch_keyset_build).  It belongs to the context that built it, remembers the modulus and the width it was built for,
// and never changes after create.  The rows hold public values only and are not wiped.
struct mpvss_modp_group_keyset {
  mpvss_ctx* ctx = nullptr;
  uint8_t q_be[RT_EB_MAX];
  size_t eb = 0;
  int lpl = 0;
  size_t n = 0;
  uint32_t* rows = nullptr;  // [n][eb / 32][16][L] words
};

namespace {

// fn(rings) with the handle's own rings: RT_NW(rings), 32, 48 or 64 words, is a compile-time constant inside fn
#define RT_NW(R) std::decay_t<decltype(R)>::NW
template <class Fn>
auto rt_rings(const mpvss_modp_group* grp, Fn fn) {
  return grp->eb == 512 ? fn(grp->r64) : grp->eb == 384 ? fn(grp->r48) : fn(grp->r32);
}

// ---- host big integers: little-endian 32-bit words, fixed capacity (2 q < 2^4098) ------------------------------
constexpr int RTW = 130;
typedef uint32_t RtNum[RTW];

void rt_from_be(RtNum x, const uint8_t* be, size_t len) {
  memset(x, 0, sizeof(RtNum));
  for (size_t i = 0; i < len; ++i) {
    const size_t bitpos = 8 * (len - 1 - i);
    x[bitpos / 32] |= (uint32_t)be[i] << (bitpos % 32);
  }
}
void rt_to_be(const RtNum x, uint8_t* be, size_t eb) {
  for (size_t i = 0; i < eb; ++i) be[eb - 1 - i] = (uint8_t)(x[i / 4] >> (8 * (i % 4)));
}
int rt_bits(const RtNum a) {
  for (int i = RTW - 1; i >= 0; --i)
    if (a[i]) return 32 * i + 32 - __builtin_clz(a[i]);
  return 0;
}
template <int NW>
void rt_to_limbs64(const RtNum x, uint64_t* v) {
  for (int i = 0; i < NW; ++i) v[i] = (uint64_t)x[2 * i] | ((uint64_t)x[2 * i + 1] << 32);
}
// 2^e mod M: products of powers of two below 2^(64 NW)
template <int NW>
void rt_pow2_mod(RtNum out, int e, const hsc::ModulusRtN<NW>& M) {
  uint64_t r[NW], t[NW];
  memset(r, 0, sizeof(r));
  r[0] = 1;
  while (e > 0) {
    const int c = e < 64 * NW - 1 ? e : 64 * NW - 1;
    memset(t, 0, sizeof(t));
    t[c / 64] = (uint64_t)1 << (c % 64);
    M.mulmod(r, r, t);
    e -= c;
  }
  memset(out, 0, sizeof(RtNum));
  for (int i = 0; i < NW; ++i) { out[2 * i] = (uint32_t)r[i]; out[2 * i + 1] = (uint32_t)(r[i] >> 32); }
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

// width of a modulus of a 256-byte handle: the smallest of 5, 9, 18 limbs per lane with bits <= 29 L - 2 (R > 4 N).  A
// 384-byte handle always runs at 27, a 512-byte one at 36.
int rt_lpl_for_bits(int bits) {
  for (int lpl : {5, 9, 18})
    if (bits <= 29 * 4 * lpl - 2) return lpl;
  return 0;
}

// the call's device copy of one image of constants, of q or of q' (context workspace, stream order)
int rt_upload(mpvss_ctx* ctx, const modp_rt_consts& image, DevBuf& buf, const modp_rt_consts** dev) {
  RET_IF(ensure(ctx, buf, sizeof(modp_rt_consts)));
  HIPCHK(ctx, hipMemcpyAsync(buf.p, &image, sizeof(modp_rt_consts), hipMemcpyHostToDevice, ctx->stream));
  *dev = (const modp_rt_consts*)buf.p;
  return 0;
}

// zero what held secrets whichever way the call ends (context lock held): device buffers in stream order, then the stream is
// drained; host vectors word by word
struct RtWipe {
  mpvss_ctx* ctx;
  std::vector<std::pair<DevBuf*, size_t>> dev;
  std::vector<std::vector<uint8_t>*> host;
  std::vector<std::pair<void*, size_t>> pinned;      // sources of asynchronous copies: zeroed once the stream is drained
  void device(DevBuf& b, size_t bytes) {               // one entry per buffer: the most bytes any chunk put there
    for (auto& d : dev)
      if (d.first == &b) { d.second = std::max(d.second, bytes); return; }
    dev.push_back({&b, bytes});
  }
  ~RtWipe() {
    for (auto* v : host) {
      volatile uint8_t* wp = v->data();
      for (size_t i = 0; i < v->size(); ++i) wp[i] = 0;
    }
    if ((!dev.empty() || !pinned.empty()) && hipSetDevice(ctx->device) == hipSuccess) {
      for (auto& d : dev)
        if (d.first->p) (void)hipMemsetAsync(d.first->p, 0, d.second < d.first->cap ? d.second : d.first->cap, ctx->stream);
      (void)hipStreamSynchronize(ctx->stream);
    }
    for (auto& pp : pinned) {
      volatile uint8_t* wp = (volatile uint8_t*)pp.first;
      for (size_t i = 0; wp && i < pp.second; ++i) wp[i] = 0;
    }
  }
};

// ---- the frame of one call (DESIGN section 13, "How a run-time entry point is put together") ------------------------------------
// An entry point checks its arguments, then constructs one RtCall with the context lock held and does everything that depends on
// `space`, on MAX_CHUNK or on what is secret through it:
//   begin()       the device, a fresh set of timing spans, and the device copies of the constants the call needs (dc, dcq);
//   for_chunks()  the one loop over MAX_CHUNK; after the body it settles the chunk unless the body did;
//   in()          a chunk of an input array on the device.  A Secret array that the frame copied there is zeroed on every way out;
//                 a caller's own device array is the caller's.  That rule is written here and nowhere else;
//   out()         where a kernel writes a chunk of an output array; settle() delivers it when the caller's array is host memory;
//   to_host()     results the host hashes, host_view() the host bytes of an input whichever space it is in;
//   settle()      the chunk's one synchronisation: outputs copied out, the stream drained, host copies handed on.
// in(), out() and their kin return null once something failed and keep the first error in `rc`: a body stages everything, checks
// `rc` once, and then launches.  A body that asks for host copies settles the chunk before it returns, failed or not, so no
// copy into its vectors outlives them.  Host vectors that hold secrets (wipe.host, host_view() of a Secret array) are declared
// BEFORE the frame, which zeroes them on its way out.
struct RtCall {
  enum Kind { Public, Secret };
  enum Consts { ModQ = 1, SubQ = 2 };                // the constants of q (dc) and of q' = (q-1)/2 (dcq)
  mpvss_ctx* const ctx;
  const mpvss_modp_group* const grp;
  const int space;
  const size_t EB;
  bool secrets_dev = false;    // Secret inputs are device arrays of the caller whatever `space` says (group_deal's device scalar ring)
  const modp_rt_consts* dc = nullptr;
  const modp_rt_consts* dcq = nullptr;
  int rc = 0;
  RtWipe wipe;

  RtCall(mpvss_ctx* c, const mpvss_modp_group* g, int sp) : ctx(c), grp(g), space(sp), EB(g->eb), wipe{c, {}, {}, {}} {}
  RtCall(const RtCall&) = delete;
  ~RtCall() {
    if (host_pending) (void)hipStreamSynchronize(ctx->stream);
  }

  // the first begin() of a call selects the device and resets the spans; each uploads the constants asked for once
  int begin(int which = ModQ) {
    if (!begun) {
      HIPCHK(ctx, hipSetDevice(ctx->device));
      spans_reset(ctx);
      begun = true;
    }
    if ((which & ModQ) && !dc) RET_IF(rt_upload(ctx, grp->c, ctx->rt_consts, &dc));
    if ((which & SubQ) && !dcq) RET_IF(rt_upload(ctx, grp->cq, ctx->rt_consts_q, &dcq));
    return 0;
  }

  template <class Body>
  int for_chunks(size_t n, Body body) {
    for (size_t off = 0; off < n; off += MAX_CHUNK) {
      settled = false;
      RET_IF(body(off, std::min(n - off, MAX_CHUNK)));
      if (!settled) RET_IF(settle());
    }
    return 0;
  }

  bool caller_on_host() const { return space != MPVSS_DEVICE; }

  const uint8_t* in(const uint8_t* arr, size_t off, size_t cnt, DevBuf& buf, Kind kind) {
    return stage(kind == Secret && secrets_dev ? MPVSS_DEVICE : space, arr + off * EB, cnt, buf, kind);
  }
  // host bytes of the library's own making (exponents it computed), whatever `space` is
  const uint8_t* in_host(const uint8_t* host, size_t cnt, DevBuf& buf, Kind kind) { return stage(MPVSS_HOST, host, cnt, buf, kind); }
  const int64_t* in_positions(const int64_t* positions, size_t off, size_t cnt) {
    const int64_t* d = nullptr;
    if (!rc) rc = stage_positions(ctx, space, positions + off, cnt, &d);
    return d;
  }

  // cnt elements of a workspace of the context; a Secret one is zeroed on the way out
  uint8_t* work(DevBuf& buf, size_t cnt, Kind kind = Public) {
    if (rc) return nullptr;
    if (kind == Secret) wipe.device(buf, cnt * EB);
    rc = ensure(ctx, buf, cnt * EB);
    return rc ? nullptr : (uint8_t*)buf.p;
  }
  // the caller's own array when it is on the device; otherwise `buf`, which settle() copies to `arr` (null: nobody wants it)
  uint8_t* out(uint8_t* arr, size_t off, size_t cnt, DevBuf& buf, Kind kind = Public) {
    if (arr && !caller_on_host()) return arr + off * EB;
    uint8_t* d = work(buf, cnt, kind);
    if (arr && d) outs.push_back({arr + off * EB, d, cnt * EB, nullptr});
    return d;
  }

  // cnt elements from the device into vec, valid after settle() or host_ready().  An out() that is read back this way reaches
  // the caller from vec: one copy over the bus, not two.
  void to_host(const uint8_t* dev, size_t cnt, std::vector<uint8_t>& vec) {
    if (rc) return;
    vec.resize(cnt * EB);
    rc = read_back(vec.data(), dev, cnt * EB);
    for (auto& o : outs)
      if (o.dev == dev) o.host = vec.data();
  }
  const uint8_t* host_view(const uint8_t* arr, size_t off, size_t cnt, std::vector<uint8_t>& vec, Kind kind = Public) {
    if (caller_on_host()) return arr + off * EB;
    if (kind == Secret && std::find(wipe.host.begin(), wipe.host.end(), &vec) == wipe.host.end()) wipe.host.push_back(&vec);
    to_host(arr + off * EB, cnt, vec);
    return vec.data();
  }
  // results that are not elements (one verdict byte, or a 32-byte challenge, per share): `bytes` of a workspace of the context, and
  // their copy into host memory, valid after settle() or host_ready() whatever `space` is
  uint8_t* raw(DevBuf& buf, size_t bytes) {
    if (rc) return nullptr;
    rc = ensure(ctx, buf, bytes);
    return rc ? nullptr : (uint8_t*)buf.p;
  }
  void host_bytes(void* host_dst, const uint8_t* dev, size_t bytes) {
    if (!rc) rc = read_back(host_dst, dev, bytes);
  }
  // before the host reads what to_host() / host_view() asked for in the middle of a chunk; nothing to wait for in host space
  int host_ready() {
    if (host_pending) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    host_pending = false;
    return rc;
  }

  // the copies of the outputs to a caller on the host, in stream order and without waiting (for a call whose end() waits)
  int flush() {
    if (rc && host_pending) (void)hipStreamSynchronize(ctx->stream);   // no copy into a body's vector outlives the body
    RET_IF(rc);
    for (auto& o : outs)
      if (!o.host) RET_IF(copy_out(ctx, space, o.dst, o.dev, o.bytes));
    return 0;
  }
  int settle() {
    RET_IF(flush());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& o : outs)
      if (o.host) memcpy(o.dst, o.host, o.bytes);
    outs.clear();
    host_pending = false;
    settled = true;
    return 0;
  }
  // the end of a call that timed its launches: the stream drained and the spans summed
  int end() { return spans_collect(ctx); }

 private:
  struct Out { uint8_t* dst; const uint8_t* dev; size_t bytes; const uint8_t* host; };
  std::vector<Out> outs;
  bool begun = false, settled = false, host_pending = false;

  const uint8_t* stage(int sp, const uint8_t* src, size_t cnt, DevBuf& buf, Kind kind) {
    if (rc) return nullptr;
    if (kind == Secret && sp != MPVSS_DEVICE) wipe.device(buf, cnt * EB);
    const void* d = nullptr;
    rc = stage_in(ctx, sp, src, cnt * EB, buf, &d);
    return (const uint8_t*)d;
  }
  int read_back(void* dst, const uint8_t* dev, size_t bytes) {
    host_pending = true;
    HIPCHK(ctx, hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
  }
};

size_t rt_L(const mpvss_modp_group* grp) { return (size_t)4 * grp->lpl; }

// 16-entry tables of `count` bases (base_stride 0: one shared base) into buf
int rt_tables(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, const uint8_t* bases_dev, size_t base_stride,
              size_t count, DevBuf& buf, const uint32_t** tab) {
  RET_IF(ensure(ctx, buf, count * 16 * rt_L(grp) * 4));
  TIMED_LAUNCH(ctx, 2, modp_rt_launch_table(grp->lpl, bases_dev, base_stride, (int)count, (uint32_t*)buf.p, dc, ctx->stream));
  *tab = (const uint32_t*)buf.p;
  return 0;
}

// a host value of the handle's element size on the device (small staging buffer of the context)
int rt_stage_small(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* host, DevBuf& buf, const uint8_t** dev) {
  RET_IF(ensure(ctx, buf, grp->eb));
  HIPCHK(ctx, hipMemcpyAsync(buf.p, host, grp->eb, hipMemcpyHostToDevice, ctx->stream));
  *dev = (const uint8_t*)buf.p;
  return 0;
}

// The batch size (shares of one call, or of one chunk) from which a call builds the fixed-base comb of a base it does not find
// in the context's cache: the build is one sequential chain of 2 044 squarings (3 068 at the wide width), and the smallest n from which build + comb
// launch is no slower than the 16-entry table + left-to-right launch it replaces is what `tools/modp_rt_rate.py --comb --ab`
// measures (profiles/modp_rt_comb_rate.txt, DESIGN section 13).  A cached comb is used at every size.  The tuning build of
// `make comb-ab` pins it with -DMPVSS_RT_COMB_MIN_SHARES=n.
#ifdef MPVSS_RT_COMB_MIN_SHARES
size_t rt_comb_min_shares(int) { return (size_t)(MPVSS_RT_COMB_MIN_SHARES); }
#else
size_t rt_comb_min_shares(int) { return 16384; }   // UNMEASURED placeholder at every width, 27 included (the twin crossover's figure)
#endif

// The one launch decision for a power of a base shared by the whole call (context lock held): the comb of (q, base) when the
// context has it; built now when the call has at least rt_comb_min_shares shares, or when `build` says so
// (mpvss_modp_group_prepare); otherwise *comb = null and the caller takes the 16-entry table of the base.  Builds run in stream
// order inside the call that needs them; calls that took the context lock are serialised, so an evicted table has no reader
// in flight.  The tables hold public values only and are not wiped.
int rt_comb_for(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, const uint8_t* base_host, size_t cnt, bool build,
                const uint32_t** comb) {
  *comb = nullptr;
  const size_t EB = grp->eb, klen = 2 * EB;               // the key is as long as the handle's (q, base): sizes never mix
  uint8_t key[2 * RT_EB_MAX];
  memcpy(key, grp->q_be, EB);
  memcpy(key + EB, base_host, EB);
  mpvss_ctx::RtComb* victim = &ctx->rt_comb[0];
  for (auto& e : ctx->rt_comb) {
    if (e.key.size() == klen && memcmp(e.key.data(), key, klen) == 0) {
      e.used = ++ctx->rt_comb_clock;
      ++ctx->rt_comb_hits;
      *comb = (const uint32_t*)e.buf.p;
      return 0;
    }
    if (!victim->key.empty() && (e.key.empty() || e.used < victim->used)) victim = &e;
  }
  if (!build && cnt < rt_comb_min_shares(grp->lpl)) return 0;
  const bool evicts = !victim->key.empty();
  victim->key.clear();                                   // no table while the build can still fail
  RET_IF(ensure(ctx, victim->buf, modp_rt_comb_bytes(grp->lpl)));
  const uint8_t* db;
  RET_IF(rt_stage_small(ctx, grp, base_host, ctx->rt_small[0], &db));
  TIMED_LAUNCH(ctx, 2, modp_rt_launch_comb_build(grp->lpl, db, (uint32_t*)victim->buf.p, dc, ctx->stream));
  victim->key.assign(key, key + klen);
  victim->used = ++ctx->rt_comb_clock;
  ++ctx->rt_comb_builds;
  if (evicts) ++ctx->rt_comb_evictions;
  *comb = (const uint32_t*)victim->buf.p;
  return 0;
}

// ---- Row layout for small calls (DESIGN section 13, "Row layout for small calls") ------------------------------------------------
// The three launches whose program exists on the row layout (modp_rt_row_kernels.hip: 16 lanes per number) go through these
// wrappers, which decide once per launch: the row kernel when the context's mode allows it (mpvss_ctx_set_rt_row), the handle
// runs at 18 / 27 / 36 limbs per lane and the count fits; the quad launch otherwise, exactly as before.  The row kernel stores
// Montgomery limbs into rt_row_m (results only), modp_rt_launch_from_mont turns them into the caller's bytes; both are timed under
// the timer of the launch they replace.
// Numbers of one launch up to which mode 1 takes the row layout: four numbers per wave on 1 024 SIMDs, one wave per SIMD -- the
// derivation of group 14's ROW_MAX_NUMBERS, not a measurement; 0: the width has no row layout.
size_t rt_row_max_shares(int lpl) { return (lpl == 18 || lpl == 27 || lpl == 36) ? 4096 : 0; }

bool rt_row_takes(mpvss_ctx* ctx, const mpvss_modp_group* grp, size_t cnt) {
  const size_t most = rt_row_max_shares(grp->lpl);
  const bool row = most != 0 && (ctx->rt_row_mode == 2 || (ctx->rt_row_mode == 1 && cnt <= most));
  ++(row ? ctx->rt_row_launches : ctx->rt_quad_launches);
  return row;
}

int rt_dual_exp_any(mpvss_ctx* ctx, const mpvss_modp_group* grp, int timer, const uint32_t* tab1, size_t tab1_stride, const uint32_t* tab2,
                    size_t tab2_stride, const uint8_t* e1, size_t e1_stride, const uint8_t* e2, size_t e2_stride, size_t cnt, uint8_t* out,
                    const modp_rt_consts* dc) {
  if (!rt_row_takes(ctx, grp, cnt)) {
    TIMED_LAUNCH(ctx, timer, modp_rt_launch_dual_exp(grp->lpl, tab1, tab1_stride, tab2, tab2_stride, e1, e1_stride, e2, e2_stride, (int)cnt,
                                                     out, dc, ctx->stream));
    return 0;
  }
  RET_IF(ensure(ctx, ctx->rt_row_m, cnt * rt_L(grp) * 4));
  uint32_t* rm = (uint32_t*)ctx->rt_row_m.p;
  TIMED_LAUNCH(ctx, timer, modp_rt_row_launch_dual_exp(grp->lpl, tab1, tab1_stride, tab2, tab2_stride, e1, e1_stride, e2, e2_stride, (int)cnt,
                                                       rm, dc, ctx->stream));
  TIMED_LAUNCH(ctx, timer, modp_rt_launch_from_mont(grp->lpl, rm, (int)cnt, out, dc, ctx->stream));
  return 0;
}

int rt_exp_sets_any(mpvss_ctx* ctx, const mpvss_modp_group* grp, int timer, const uint32_t* tab, size_t tab_stride, const uint8_t* e1,
                    const uint8_t* e2, size_t cnt, uint8_t* out1, uint8_t* out2, const modp_rt_consts* dc) {
  if (!rt_row_takes(ctx, grp, cnt)) {
    TIMED_LAUNCH(ctx, timer, modp_rt_launch_exp_sets(grp->lpl, tab, tab_stride, e1, e2, (int)cnt, out1, out2, dc, ctx->stream));
    return 0;
  }
  RET_IF(ensure(ctx, ctx->rt_row_m, 2 * cnt * rt_L(grp) * 4));
  uint32_t* rm = (uint32_t*)ctx->rt_row_m.p;
  TIMED_LAUNCH(ctx, timer, modp_rt_row_launch_exp_sets(grp->lpl, tab, tab_stride, e1, e2, (int)cnt, rm, dc, ctx->stream));
  TIMED_LAUNCH(ctx, timer, modp_rt_launch_from_mont(grp->lpl, rm, (int)cnt, out1, dc, ctx->stream));
  TIMED_LAUNCH(ctx, timer, modp_rt_launch_from_mont(grp->lpl, rm + cnt * rt_L(grp), (int)cnt, out2, dc, ctx->stream));
  return 0;
}

int rt_comb_exp_any(mpvss_ctx* ctx, const mpvss_modp_group* grp, int timer, const uint32_t* comb, const uint32_t* tab2, size_t tab2_stride,
                    const uint8_t* e1, const uint8_t* e2, size_t e2_stride, size_t cnt, uint8_t* out, const modp_rt_consts* dc) {
  if (!rt_row_takes(ctx, grp, cnt)) {
    TIMED_LAUNCH(ctx, timer, modp_rt_launch_comb_exp(grp->lpl, comb, tab2, tab2_stride, e1, e2, e2_stride, (int)cnt, out, dc, ctx->stream));
    return 0;
  }
  RET_IF(ensure(ctx, ctx->rt_row_m, cnt * rt_L(grp) * 4));
  uint32_t* rm = (uint32_t*)ctx->rt_row_m.p;
  TIMED_LAUNCH(ctx, timer, modp_rt_row_launch_comb_exp(grp->lpl, comb, tab2, tab2_stride, e1, e2, e2_stride, (int)cnt, rm, dc, ctx->stream));
  TIMED_LAUNCH(ctx, timer, modp_rt_launch_from_mont(grp->lpl, rm, (int)cnt, out, dc, ctx->stream));
  return 0;
}

// a1 = g1^r h1^c and a2 = g2^r h2^c for cnt shares (device pointers but g1: one shared base in host bytes; c stride 0 = shared);
// g2: the second proof's bases as bytes, or (g2 null) g2_rows: the rows of a key set from the chunk's first key on -- or, with
// g2_key_of, from the set's first key on, share i taking key g2_key_of[i] (device; a run of boxes of mpvss_modp_group_verify_many)
int rt_dleq_dev(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, const uint8_t* g1_host, const uint8_t* h1,
                const uint8_t* g2, const uint32_t* g2_rows, const uint8_t* h2, const uint8_t* r, const uint8_t* c, size_t c_stride,
                size_t cnt, uint8_t* a1, uint8_t* a2, const uint32_t* g2_key_of = nullptr) {
  const size_t TW = 16 * rt_L(grp), EB = grp->eb;
  const uint32_t *tg, *t1, *t2;
  if (a1) {
    RET_IF(rt_comb_for(ctx, grp, dc, g1_host, cnt, false, &tg));
    RET_IF(rt_tables(ctx, grp, dc, h1, EB, cnt, ctx->rt_tab1, &t1));
    if (tg) {
      RET_IF(rt_comb_exp_any(ctx, grp, 1, tg, t1, TW, r, c, c_stride, cnt, a1, dc));
    } else {
      const uint8_t* dg1;
      RET_IF(rt_stage_small(ctx, grp, g1_host, ctx->rt_small[0], &dg1));
      RET_IF(rt_tables(ctx, grp, dc, dg1, 0, 1, ctx->rt_tabg, &tg));
      RET_IF(rt_dual_exp_any(ctx, grp, 1, tg, 0, t1, TW, r, EB, c, c_stride, cnt, a1, dc));
    }
  }
  if (a2) {
    RET_IF(rt_tables(ctx, grp, dc, h2, EB, cnt, ctx->rt_tab2, &t2));
    if (g2) {
      RET_IF(rt_tables(ctx, grp, dc, g2, EB, cnt, ctx->rt_tab1, &t1));
      RET_IF(rt_dual_exp_any(ctx, grp, 3, t1, TW, t2, TW, r, EB, c, c_stride, cnt, a2, dc));
    } else if (g2_key_of) {
      TIMED_LAUNCH(ctx, 3, modp_rt_launch_keyset_exp_idx(grp->lpl, g2_rows, g2_key_of, t2, TW, r, c, c_stride, (int)cnt, a2, dc, ctx->stream));
    } else {
      TIMED_LAUNCH(ctx, 3, modp_rt_launch_keyset_exp(grp->lpl, g2_rows, t2, TW, r, nullptr, c, c_stride, (int)cnt, a2, nullptr, dc,
                                                     ctx->stream));
    }
  }
  return 0;
}

// ---- X_i: Horner's rule, or forward differences in the exponent (DESIGN section 13, "Forward differences") ---------------------
// Chains a call of n consecutive positions is cut into, and the batch size (shares of one call, or of one chunk) from which
// mode 1 takes forward differences.  Both come from `tools/modp_rt_rate.py --fd --ab` (profiles/modp_rt_fd_rate.txt).
// Seeds cost 2 S t Horner evaluations at low occupancy, a chain 3 (t - 1) product latencies of set-up and n / (2 S) of
// stepping per direction: more chains shorten the stepping until the seeds fill the chip.
int rt_fd_chains(int, size_t n, size_t t) {
  const size_t s = n / (4 * t);
  return (int)(s < 1 ? 1 : s > 32 ? 32 : s);
}
size_t rt_fd_min_shares(int, size_t t) { return std::max<size_t>(16384, 8 * t); }
// mode 1 of mpvss_ctx_set_rt_fd.  The gate of the forward differences (at most half of Horner's time at (65 536, 256) and 2048
// bits) is judged in DESIGN section 13 from profiles/modp_rt_fd_rate.txt; until it is met "automatic" means Horner.
constexpr bool RT_FD_AUTO_ON = false;

// Once per call, after rt_stage_commitments: the inverted commitments in Montgomery form (ctx->rt_cm_inv), by Montgomery's
// trick on the host -- one inversion mod q and 3 (t - 1) products.  Leaves ctx->rt_fd_ready false, and the call with Horner,
// when the mode, t, the call's size or a commitment that is no unit mod q rules forward differences out.
int rt_fd_prepare(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, int space, const uint8_t* commitments,
                  size_t t, size_t n) {
  ctx->rt_fd_ready = false;
  const int mode = ctx->rt_fd_mode;
  const size_t most = std::min(n, MAX_CHUNK), EB = grp->eb;
  if (mode == 0 || (mode == 1 && !RT_FD_AUTO_ON) || t < 2 || t > (size_t)modp_rt_fd_max_t(grp->lpl) || most < t) return 0;
  if (mode == 1 && most < rt_fd_min_shares(grp->lpl, t)) return 0;
  std::vector<uint8_t> back;
  const uint8_t* C = commitments;
  if (space == MPVSS_DEVICE) {
    back.resize(t * EB);
    HIPCHK(ctx, hipMemcpyAsync(back.data(), commitments, t * EB, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    C = back.data();
  }
  ctx->rt_fd_inv_host.resize(t * EB);
  uint8_t* inv = ctx->rt_fd_inv_host.data();
  const bool units = rt_rings(grp, [&](const auto& R) {
    constexpr int NW = RT_NW(R);
    std::vector<uint64_t> v(t * NW), pre(t * NW);
    for (size_t j = 0; j < t; ++j) {
      hsc::from_bytes<NW>(&v[j * NW], C + j * EB, true);
      R.mod.reduce1(&v[j * NW]);
      if (j == 0) memcpy(&pre[0], &v[0], NW * 8);
      else R.mod.mulmod(&pre[j * NW], &pre[(j - 1) * NW], &v[j * NW]);
    }
    uint64_t run[NW], x[NW];
    if (!R.mod.invert(run, &pre[(t - 1) * NW])) return false;      // some commitment is 0 or shares a factor with q
    for (size_t j = t - 1; j > 0; --j) {
      R.mod.mulmod(x, run, &pre[(j - 1) * NW]);
      hsc::to_bytes<NW>(inv + j * EB, x, true);
      R.mod.mulmod(run, run, &v[j * NW]);
    }
    hsc::to_bytes<NW>(inv, run, true);
    return true;
  });
  if (!units) return 0;
  RET_IF(ensure(ctx, ctx->rt_fd_inv, t * EB));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_fd_inv.p, inv, t * EB, hipMemcpyHostToDevice, ctx->stream));
  RET_IF(ensure(ctx, ctx->rt_cm_inv, t * rt_L(grp) * 4));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, (const uint8_t*)ctx->rt_fd_inv.p, (int)t, (uint32_t*)ctx->rt_cm_inv.p, dc, ctx->stream));
  ctx->rt_fd_ready = true;
  return 0;
}

// The admissibility of one chunk, on the host: cnt positions (in `space`) that are p0, p0 + 1, .. with p0 >= 0, all of them below
// q - 1 when that fits 64 bits (Horner reduces a position mod q - 1, forward differences use it as an integer).
int rt_fd_positions_ok(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const int64_t* positions, size_t cnt, bool* ok,
                       int64_t* p0_out) {
  *ok = false;
  std::vector<int64_t> back;
  const int64_t* P = positions;
  if (space == MPVSS_DEVICE) {
    back.resize(cnt);
    HIPCHK(ctx, hipMemcpyAsync(back.data(), positions, cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    P = back.data();
  }
  const int64_t p0 = P[0];
  if (p0 < 0 || p0 > INT64_MAX - (int64_t)(cnt - 1)) return 0;
  for (size_t i = 1; i < cnt; ++i)
    if (P[i] != p0 + (int64_t)i) return 0;
  const uint64_t qm1 = ((uint64_t)grp->c.qm1_hi << 32) | grp->c.qm1_lo;
  if (qm1 != 0 && (uint64_t)p0 + (cnt - 1) >= qm1) return 0;
  *p0_out = p0;
  *ok = true;
  return 0;
}

// X_i of cnt shares (commitments already in ctx->rt_cm, Montgomery form; `positions`: the chunk's positions as the caller
// gave them, in `space`).  THE launch decision of the X path, on the host before anything is launched: forward differences
// when the call has inverted commitments (rt_fd_prepare), the chunk is large enough for its mode and its positions are
// admissible; otherwise k_rt_commit_eval.  Under these conditions the recurrences are integer identities in the exponent,
// so both paths give the same bytes.
int rt_commit_eval_dev(RtCall& f, size_t t, const int64_t* pos_dev, size_t cnt, uint8_t* x_dev, const int64_t* positions) {
  mpvss_ctx* const ctx = f.ctx;
  const mpvss_modp_group* const grp = f.grp;
  const modp_rt_consts* const dc = f.dc;
  const size_t LW = rt_L(grp);
  bool fd = ctx->rt_fd_ready && cnt >= t && (ctx->rt_fd_mode == 2 || cnt >= rt_fd_min_shares(grp->lpl, t)) &&
            cnt * LW * 4 <= ((size_t)1 << 30);               // X in limbs stays a workspace of at most 1 GiB
  int64_t p0 = 0;
  if (fd) RET_IF(rt_fd_positions_ok(ctx, grp, f.space, positions, cnt, &fd, &p0));
  if (!fd) {
    ++ctx->rt_horner_calls;
    TIMED_LAUNCH(ctx, 0, modp_rt_launch_commit_eval(grp->lpl, (const uint32_t*)ctx->rt_cm.p, (int)t, pos_dev, (int)cnt, x_dev, dc,
                                                    ctx->stream));
    return 0;
  }
  ++ctx->rt_fd_calls;
  size_t S = ctx->rt_fd_chains > 0 ? (size_t)ctx->rt_fd_chains : (size_t)rt_fd_chains(grp->lpl, cnt, t);
  S = std::max<size_t>(1, std::min(S, cnt / t));             // every chain holds at least t positions
  std::vector<int64_t>& sp = ctx->rt_fd_pos_host;
  sp.resize(S * t);
  for (size_t c = 0; c < S; ++c) {
    int first, len;
    modp_rt_fd_chain((int)cnt, (int)S, (int)c, &first, &len);
    for (size_t k = 0; k < t; ++k) sp[c * t + k] = p0 + first + (len - (int)t) / 2 + (int64_t)k;
  }
  RET_IF(ensure(ctx, ctx->rt_fd_pos, S * t * 8));
  RET_IF(ensure(ctx, ctx->rt_fd_seeds, 2 * S * t * LW * 4));
  RET_IF(ensure(ctx, ctx->rt_fd_x, cnt * LW * 4));
  RET_IF(ensure(ctx, ctx->rt_fd_park, modp_rt_fd_park_bytes(grp->lpl, (int)t, (int)S)));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_fd_pos.p, sp.data(), S * t * 8, hipMemcpyHostToDevice, ctx->stream));
  uint32_t* seeds = (uint32_t*)ctx->rt_fd_seeds.p;
  uint32_t* xm = (uint32_t*)ctx->rt_fd_x.p;
  RET_IF(span_begin(ctx, 0));
  LAUNCHCHK(ctx, modp_rt_launch_commit_eval_mont(grp->lpl, (const uint32_t*)ctx->rt_cm.p, (const uint32_t*)ctx->rt_cm_inv.p, (int)t,
                                                 (const int64_t*)ctx->rt_fd_pos.p, (int)(S * t), seeds, dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_fd_chains(grp->lpl, seeds, (int)t, (int)cnt, (int)S, xm, (uint32_t*)ctx->rt_fd_park.p, dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_from_mont(grp->lpl, xm, (int)cnt, x_dev, dc, ctx->stream));
  RET_IF(span_end(ctx));
  return 0;
}

int rt_stage_commitments(RtCall& f, const uint8_t* commitments, size_t t, size_t n) {
  mpvss_ctx* const ctx = f.ctx;
  const uint8_t* dcm = f.in(commitments, 0, t, ctx->rt_in[4], RtCall::Public);
  RET_IF(f.rc);
  RET_IF(ensure(ctx, ctx->rt_cm, t * rt_L(f.grp) * 4));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(f.grp->lpl, dcm, (int)t, (uint32_t*)ctx->rt_cm.p, f.dc, ctx->stream));
  return rt_fd_prepare(ctx, f.grp, f.dc, f.space, commitments, t, n);
}

// hash_to_scalar of the group: int(SHA-256(data)) mod (q-1)/2, big-endian at the handle's element size
void rt_hash_to_scalar(const mpvss_modp_group* grp, const uint8_t* data, size_t len, uint8_t* out) {
  const size_t EB = grp->eb;
  uint8_t h[RT_EB_MAX];
  memset(h, 0, EB - 32);
  mpvss::sha256(data, len, h + EB - 32);
  rt_rings(grp, [&](const auto& R) {
    constexpr int NW = RT_NW(R);
    uint64_t x[NW];
    hsc::from_bytes<NW>(x, h, true);
    R.sub.reduce1(x);
    hsc::to_bytes<NW>(out, x, true);
  });
}

// the challenge of one share's DLEQ proof: hash_to_scalar(SHA-256(framed(a) | framed(b) | framed(a1) | framed(a2))), dleq.rs:119-126
void rt_share_challenge(const mpvss_modp_group* grp, const uint8_t* a, const uint8_t* b, const uint8_t* a1, const uint8_t* a2,
                        uint8_t* out) {
  mpvss::Sha256 hs;
  for (const uint8_t* e : {a, b, a1, a2}) frame_update(hs, e, grp->eb);
  uint8_t digest[32];
  hs.final(digest);
  rt_hash_to_scalar(grp, digest, 32, out);
}

// THE launch decision of the per-share hash for one whole call of n shares (defined beside rt_scalar_on_device); counts the call
bool rt_share_hash_on_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, size_t n);

// The same challenges for cnt shares on the device (k_rt_share_verdict, timer 5; all pointers device memory, arrays [cnt][EB]).
// c_out null: verdict[i] = (c_i == challenge_i); c_out given: challenge_i as c_out_stride (32 or EB) bytes.  For handles with
// has_sh only: the kernel leaves out the reduction mod (q-1)/2, which is the identity there.
int rt_share_hash_dev(RtCall& f, const uint8_t* a, const uint8_t* b, const uint8_t* a1, const uint8_t* a2, const uint8_t* c, size_t cnt,
                      uint8_t* verdict, uint8_t* c_out, size_t c_out_stride) {
  TIMED_LAUNCH(f.ctx, 5, verdict_launch_rt((int)f.EB, a, b, a1, a2, c, (int)cnt, verdict, c_out, (int)c_out_stride, f.ctx->stream));
  return 0;
}
// 32-byte challenges as they crossed the bus -> EB-byte big-endian scalars
void rt_widen_challenges(const uint8_t* c32, size_t cnt, size_t EB, uint8_t* out) {
  for (size_t i = 0; i < cnt; ++i) {
    memset(out + i * EB, 0, EB - 32);
    memcpy(out + i * EB + EB - 32, c32 + i * 32, 32);
  }
}
const char* const RT_NO_SH = "the handle has no device share hash: (q-1)/2 is below 2^256 (mpvss_modp_group_has_device_share_hash)";

bool rt_bad_group(const mpvss_modp_group* grp) { return grp == nullptr || grp->lpl == 0; }

// words of one key's rows
size_t rt_keyset_stride(const mpvss_modp_group* grp) { return modp_rt_keyset_bytes(grp->lpl, 1) / 4; }

// The one admission of a key set to a call (context lock held): built by this context, for this modulus at this width, and
// holding the keys key_offset .. key_offset + n - 1.  *rows: the rows of key key_offset.
// Why not, or null when the set is admitted (mpvss_modp_group_verify_many asks without failing the call).
const char* rt_keyset_refusal(const mpvss_ctx* ctx, const mpvss_modp_group* grp, const mpvss_modp_group_keyset* ks, size_t key_offset,
                              size_t n) {
  if (!ks) return "key set: none given";
  if (ks->ctx != ctx) return "key set: built by another context";
  if (ks->eb != grp->eb || ks->lpl != grp->lpl || memcmp(ks->q_be, grp->q_be, grp->eb) != 0) return "key set: built for another modulus";
  if (key_offset > ks->n || n > ks->n - key_offset) return "key set: key_offset + n is beyond the set";
  return nullptr;
}
int rt_keyset_rows(mpvss_ctx* ctx, const mpvss_modp_group* grp, const mpvss_modp_group_keyset* ks, size_t key_offset, size_t n,
                   const uint32_t** rows) {
  if (const char* why = rt_keyset_refusal(ctx, grp, ks, key_offset, n)) return fail(ctx, MPVSS_E_INVALID, why);
  *rows = ks->rows + key_offset * rt_keyset_stride(grp);
  return 0;
}

}  // namespace

namespace {

// the handle of an odd q >= 5 of `bits` bits at element size eb and lpl limbs per lane
template <int NW>
int rt_group_build(const RtNum q, int bits, size_t eb, int lpl, RtRings<NW> mpvss_modp_group::*rings, mpvss_modp_group** out) {
  mpvss_modp_group* g = new (std::nothrow) mpvss_modp_group();
  if (!g) return MPVSS_E_NOMEM;
  memset(&g->c, 0, sizeof(g->c));
  g->bits = bits;
  g->lpl = lpl;
  g->eb = eb;
  RtRings<NW>& R = g->*rings;
  const int L = 4 * g->lpl;
  const int in_rows = modp_rt_in_rows(g->lpl);
  rt_limbs(q, g->c.n, L);
  uint64_t q64[NW];
  rt_to_limbs64<NW>(q, q64);
  R.mod.set(q64);
  q64[0] -= 1;                                   // q is odd
  R.ord.set(q64);
  for (int i = 0; i < NW; ++i) q64[i] = (q64[i] >> 1) | (i + 1 < NW ? q64[i + 1] << 63 : 0);
  R.sub.set(q64);
  rt_to_be(q, g->q_be, eb);
  RtNum k;
  rt_pow2_mod<NW>(k, 29 * (in_rows + L), R.mod);
  rt_limbs(k, g->c.kin, L);
  rt_pow2_mod<NW>(k, 29 * L, R.mod);
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
  rt_to_be(sub, g->sub_be, eb);
  memset(g->g_be, 0, sizeof(g->g_be));
  g->g_be[eb - 1] = 4;
  memset(g->G_be, 0, sizeof(g->G_be));
  g->G_be[eb - 1] = 2;
  // the constants of q' for the device-side scalar ring: q' odd (q = 3 mod 4) and q' >= 3 (q >= 7) -- every safe prime above 5
  memset(&g->cq, 0, sizeof(g->cq));
  memset(g->subR_be, 0, sizeof(g->subR_be));
  memset(g->subm2_be, 0, sizeof(g->subm2_be));
  g->has_q = (q[0] & 3) == 3 && (bits > 3 || q[0] >= 7);
  g->has_sh = bits >= 258;                       // q odd: (q-1)/2 >= 2^256  <=>  q >= 2^257 + 1  <=>  bits(q) >= 258
  if (g->has_q) {
    rt_limbs(sub, g->cq.n, L);
    rt_pow2_mod<NW>(k, 29 * (in_rows + L), R.sub);
    rt_limbs(k, g->cq.kin, L);
    rt_pow2_mod<NW>(k, 29 * L, R.sub);
    rt_limbs(k, g->cq.one_m, L);
    rt_to_be(k, g->subR_be, eb);
    RtNum m2;                                    // q' - 2 (q' >= 3)
    memcpy(m2, sub, sizeof(RtNum));
    for (int i = 0, borrow = 2; i < RTW && borrow; ++i) {
      const uint32_t before = m2[i];
      m2[i] -= (uint32_t)borrow;
      borrow = before < (uint32_t)borrow ? 1 : 0;
    }
    rt_to_be(m2, g->subm2_be, eb);
    g->cq.one[0] = 1;
    uint32_t qinv = sub[0];
    for (int i = 0; i < 5; ++i) qinv *= 2u - sub[0] * qinv;
    g->cq.n0inv = (0u - qinv) & ((1u << 29) - 1);
    g->cq.lpl = (uint32_t)g->lpl;
  }
  *out = g;
  return MPVSS_OK;
}

// q of at most max_bytes significant bytes, odd and >= 5; its bit length, or 0
int rt_parse_modulus(const uint8_t* q_be, size_t q_len, size_t max_bytes, RtNum q) {
  if (!q_be) return 0;
  size_t skip = 0;
  while (skip < q_len && q_be[skip] == 0) ++skip;          // leading zero bytes are allowed
  if (q_len - skip > max_bytes) return 0;
  rt_from_be(q, q_be + skip, q_len - skip);
  const int bits = rt_bits(q);
  if (bits == 0 || (q[0] & 1) == 0 || (bits <= 3 && q[0] < 5)) return 0;   // even, or below 5
  return bits;
}

}  // namespace

extern "C" int mpvss_modp_group_create(const uint8_t* q_be, size_t q_len, mpvss_modp_group** out) {
  if (!out) return MPVSS_E_INVALID;
  *out = nullptr;
  RtNum q;
  const int bits = rt_parse_modulus(q_be, q_len, MPVSS_MODP_BYTES, q);     // more than 2048 bits: mpvss_modp_group_create_wide
  if (bits == 0) return MPVSS_E_INVALID;
  return rt_group_build<32>(q, bits, MPVSS_MODP_BYTES, rt_lpl_for_bits(bits), &mpvss_modp_group::r32, out);
}

extern "C" int mpvss_modp_group_create_wide(const uint8_t* q_be, size_t q_len, size_t elem_bytes, mpvss_modp_group** out) {
  if (!out) return MPVSS_E_INVALID;
  *out = nullptr;
  if (elem_bytes == MPVSS_MODP_BYTES) return mpvss_modp_group_create(q_be, q_len, out);
  if (elem_bytes != 384 && elem_bytes != 512) return MPVSS_E_INVALID;
  RtNum q;
  const int bits = rt_parse_modulus(q_be, q_len, elem_bytes, q);
  if (bits <= 8 * ((int)elem_bytes - 128)) return MPVSS_E_INVALID;         // the next narrower handle serves it (or q is no modulus)
  if (elem_bytes == 512) return rt_group_build<64>(q, bits, 512, 36, &mpvss_modp_group::r64, out);
  return rt_group_build<48>(q, bits, 384, 27, &mpvss_modp_group::r48, out);
}

extern "C" void mpvss_modp_group_destroy(mpvss_modp_group* grp) { delete grp; }

extern "C" int mpvss_modp_group_bits(const mpvss_modp_group* grp) { return grp ? grp->bits : MPVSS_E_INVALID; }

extern "C" int mpvss_modp_group_limbs_per_lane(const mpvss_modp_group* grp) { return grp ? grp->lpl : MPVSS_E_INVALID; }

extern "C" int mpvss_modp_group_elem_bytes(const mpvss_modp_group* grp) { return grp ? (int)grp->eb : MPVSS_E_INVALID; }

extern "C" int mpvss_modp_group_hash_to_scalar(const mpvss_modp_group* grp, const uint8_t* data, size_t len, uint8_t* out256) {
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
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* db = f.in(bases, off, cnt, ctx->rt_in[0], RtCall::Public);
    const uint8_t* de = f.in(exps, off, cnt, ctx->rt_in[1], RtCall::Public);
    uint8_t* dout = f.out(out, off, cnt, ctx->rt_out[0]);
    RET_IF(f.rc);
    const uint32_t* t1;
    RET_IF(rt_tables(ctx, grp, f.dc, db, f.EB, cnt, ctx->rt_tab1, &t1));
    RET_IF(rt_dual_exp_any(ctx, grp, 3, t1, 16 * rt_L(grp), nullptr, 0, de, f.EB, nullptr, 0, cnt, dout, f.dc));
    return 0;
  }));
  return f.end();
}

extern "C" int mpvss_modp_group_batch_mul(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* a, const uint8_t* b,
                                          size_t n, uint8_t* out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_batch_mul: no group");
  if (n == 0) return MPVSS_OK;
  if (!a || !b || !out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_batch_mul: bad argument");
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  const uint8_t* da = f.in(a, 0, n, ctx->rt_in[0], RtCall::Public);
  const uint8_t* db = f.in(b, 0, n, ctx->rt_in[1], RtCall::Public);
  uint8_t* dout = f.out(out, 0, n, ctx->rt_out[0]);
  RET_IF(f.rc);
  const size_t LW = rt_L(grp);
  RET_IF(ensure(ctx, ctx->rt_tab1, n * LW * 4));
  RET_IF(ensure(ctx, ctx->rt_tab2, n * LW * 4));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, da, (int)n, (uint32_t*)ctx->rt_tab1.p, f.dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, db, (int)n, (uint32_t*)ctx->rt_tab2.p, f.dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_mul(grp->lpl, (const uint32_t*)ctx->rt_tab1.p, (const uint32_t*)ctx->rt_tab2.p, (int)n, dout, f.dc,
                                    ctx->stream));
  return f.settle();
}

extern "C" int mpvss_modp_group_commit_eval(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments,
                                            size_t t, const int64_t* positions, size_t n, uint8_t* x_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_commit_eval: no group");
  if (n == 0) return MPVSS_OK;
  if (!commitments || !positions || !x_out || t == 0 || t > 0x7fffffff || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_commit_eval: bad argument (t must be >= 1)");
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  RET_IF(rt_stage_commitments(f, commitments, t, n));
  const int64_t* dpos = f.in_positions(positions, 0, n);
  uint8_t* dout = f.out(x_out, 0, n, ctx->rt_out[0]);
  RET_IF(f.rc);
  RET_IF(rt_commit_eval_dev(f, t, dpos, n, dout, positions));
  RET_IF(f.flush());
  return f.end();
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
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  const uint8_t* dcc = nullptr;
  if (!c_per_share) RET_IF(rt_stage_small(ctx, grp, c, ctx->rt_small[1], &dcc));
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* dh1 = f.in(h1, off, cnt, ctx->rt_in[0], RtCall::Public);
    const uint8_t* dg2 = f.in(g2, off, cnt, ctx->rt_in[1], RtCall::Public);
    const uint8_t* dh2 = f.in(h2, off, cnt, ctx->rt_in[2], RtCall::Public);
    const uint8_t* dr = f.in(r, off, cnt, ctx->rt_in[3], RtCall::Public);
    const uint8_t* dcs = c_per_share ? f.in(c, off, cnt, ctx->rt_in[5], RtCall::Public) : dcc;
    uint8_t* d1 = f.out(a1_out, off, cnt, ctx->rt_out[0]);
    uint8_t* d2 = f.out(a2_out, off, cnt, ctx->rt_out[1]);
    RET_IF(f.rc);
    return rt_dleq_dev(ctx, grp, f.dc, g1_host, dh1, dg2, nullptr, dh2, dr, dcs, c_per_share ? f.EB : 0, cnt, d1, d2);
  }));
  return f.end();
}

namespace {
// participant.rs:399-455 for one box, arguments checked and the context lock held: the keys are the caller's array `pubkeys`, or
// (pubkeys null) key_rows, the rows of a key set from the box's first key on
int rt_verify_distribution_locked(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments, size_t t,
                                  const int64_t* positions, const uint8_t* pubkeys, const uint32_t* key_rows, const uint8_t* shares,
                                  const uint8_t* responses, size_t n, const uint8_t* challenge_host, int* verdict,
                                  uint8_t* digest32_out, uint8_t* x_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host) {
  const size_t EB = grp->eb;
  *verdict = 0;
  mpvss::Sha256 h;
  if (n > 0) {
    std::vector<uint8_t> hX, hY, h1, h2;
    RtCall f(ctx, grp, space);
    RET_IF(f.begin());
    RET_IF(rt_stage_commitments(f, commitments, t, n));
    const uint8_t* dch;
    RET_IF(rt_stage_small(ctx, grp, challenge_host, ctx->rt_small[1], &dch));
    RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
      const int64_t* dpos = f.in_positions(positions, off, cnt);
      const uint8_t* dy = pubkeys ? f.in(pubkeys, off, cnt, ctx->rt_in[1], RtCall::Public) : nullptr;
      const uint8_t* dY = f.in(shares, off, cnt, ctx->rt_in[2], RtCall::Public);
      const uint8_t* dr = f.in(responses, off, cnt, ctx->rt_in[3], RtCall::Public);
      uint8_t* dX = f.work(ctx->rt_out[0], cnt);
      uint8_t* d1 = f.work(ctx->rt_out[1], cnt);
      uint8_t* d2 = f.work(ctx->rt_out[2], cnt);
      RET_IF(f.rc);
      RET_IF(rt_commit_eval_dev(f, t, dpos, cnt, dX, positions + off));
      // a1 = g^r X^c, a2 = y^r Y^c (src/participant.rs:436-447 -> src/dleq.rs:66-84)
      RET_IF(rt_dleq_dev(ctx, grp, f.dc, grp->g_be, dX, dy, pubkeys ? nullptr : key_rows + off * rt_keyset_stride(grp), dY, dr, dch, 0,
                         cnt, d1, d2));
      f.to_host(dX, cnt, hX);
      f.to_host(d1, cnt, h1);
      f.to_host(d2, cnt, h2);
      const uint8_t* Y = f.host_view(shares, off, cnt, hY);
      RET_IF(f.settle());
      // the transcript hashes Y_i as the box carries it (src/participant.rs:448), X_i, a1_i, a2_i canonical
      frame_shares(h, hX.data(), Y, h1.data(), h2.data(), 0, cnt, EB);
      if (x_out_host) memcpy(x_out_host + off * EB, hX.data(), cnt * EB);
      if (a1_out_host) memcpy(a1_out_host + off * EB, h1.data(), cnt * EB);
      if (a2_out_host) memcpy(a2_out_host + off * EB, h2.data(), cnt * EB);
      return 0;
    }));
    RET_IF(f.end());
  }
  uint8_t digest[32], c[RT_EB_MAX];
  h.final(digest);
  if (digest32_out) memcpy(digest32_out, digest, 32);
  rt_hash_to_scalar(grp, digest, 32, c);          // src/participant.rs:451-455
  *verdict = memcmp(c, challenge_host, EB) == 0 ? 1 : 0;
  return MPVSS_OK;
}
}  // namespace

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
  return rt_verify_distribution_locked(ctx, grp, space, commitments, t, positions, pubkeys, nullptr, shares, responses, n, challenge_host,
                                       verdict, digest32_out, x_out_host, a1_out_host, a2_out_host);
}

extern "C" int mpvss_modp_group_verify_shares(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* pk,
                                              const uint8_t* s, const uint8_t* y, const uint8_t* c, const uint8_t* r, size_t n,
                                              uint8_t* verdicts_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_verify_shares: no group");
  const size_t EB = grp->eb;
  if (n == 0) return MPVSS_OK;
  if (!pk || !s || !y || !c || !r || !verdicts_host || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_verify_shares: bad argument");
  std::vector<uint8_t> hpk, hY, hc, h1, h2;
  RtCall f(ctx, grp, space);
  const bool hdev = rt_share_hash_on_device(ctx, grp, n);
  RET_IF(f.begin());
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* dpk = f.in(pk, off, cnt, ctx->rt_in[0], RtCall::Public);
    const uint8_t* ds = f.in(s, off, cnt, ctx->rt_in[1], RtCall::Public);
    const uint8_t* dy = f.in(y, off, cnt, ctx->rt_in[2], RtCall::Public);
    const uint8_t* dcc = f.in(c, off, cnt, ctx->rt_in[5], RtCall::Public);
    const uint8_t* dr = f.in(r, off, cnt, ctx->rt_in[3], RtCall::Public);
    uint8_t* d1 = f.work(ctx->rt_out[1], cnt);
    uint8_t* d2 = f.work(ctx->rt_out[2], cnt);
    uint8_t* dv = hdev ? f.raw(ctx->rt_sh_verdict, cnt) : nullptr;
    RET_IF(f.rc);
    // a1 = G^r pk^c, a2 = S^r Y^c (src/participant.rs:361-386 -> src/dleq.rs:275-302)
    RET_IF(rt_dleq_dev(ctx, grp, f.dc, grp->G_be, dpk, ds, nullptr, dy, dr, dcc, EB, cnt, d1, d2));
    if (hdev) {                                  // a1 and a2 stay where they are; the chunk's verdict bytes alone cross the bus
      RET_IF(rt_share_hash_dev(f, dpk, dy, d1, d2, dcc, cnt, dv, nullptr, 0));
      f.host_bytes(verdicts_host + off, dv, cnt);
      return f.rc;
    }
    f.to_host(d1, cnt, h1);
    f.to_host(d2, cnt, h2);
    const uint8_t* P = f.host_view(pk, off, cnt, hpk);
    const uint8_t* Y = f.host_view(y, off, cnt, hY);
    const uint8_t* C = f.host_view(c, off, cnt, hc);
    RET_IF(f.settle());
    for (size_t i = 0; i < cnt; ++i) {
      uint8_t cc[RT_EB_MAX];
      rt_share_challenge(grp, P + i * EB, Y + i * EB, h1.data() + i * EB, h2.data() + i * EB, cc);
      verdicts_host[off + i] = memcmp(cc, C + i * EB, EB) == 0 ? 1 : 0;
    }
    return 0;
  }));
  return f.end();
}

// =====================================================================================================================
// The rest of the protocol for a run-time group: the scalar ring Z/(q-1) on the host (and, further down, on the device), the dealer (distribute / deal),
// extract_secret_share and reconstruct.
// =====================================================================================================================

// ---- scalar ring (host only, no context): the group-14 contracts of capi_scalar.inc with q - 1 of the handle ---------------
extern "C" int mpvss_modp_group_scalar_mul(const mpvss_modp_group* grp, const uint8_t* a256, const uint8_t* b256, uint8_t* out256) {
  if (rt_bad_group(grp) || !a256 || !b256 || !out256) return MPVSS_E_INVALID;
  rt_rings(grp, [&](const auto& R) { scalar_mul_bytes<RT_NW(R)>(R.ord, true, a256, b256, out256); });   // modp.rs:180-182
  return MPVSS_OK;
}
extern "C" int mpvss_modp_group_scalar_sub(const mpvss_modp_group* grp, const uint8_t* a256, const uint8_t* b256, uint8_t* out256) {
  if (rt_bad_group(grp) || !a256 || !b256 || !out256) return MPVSS_E_INVALID;
  rt_rings(grp, [&](const auto& R) { scalar_sub_bytes<RT_NW(R)>(R.ord, true, a256, b256, out256); });   // modp.rs:184-192
  return MPVSS_OK;
}
extern "C" int mpvss_modp_group_dleq_responses(const mpvss_modp_group* grp, const uint8_t* w, const uint8_t* alpha, const uint8_t* c,
                                               int c_per_share, size_t n, uint8_t* r_out, int threads) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  if (n == 0) return MPVSS_OK;
  if (!w || !alpha || !c || !r_out) return MPVSS_E_INVALID;
  rt_rings(grp, [&](const auto& R) {
    responses_bytes<RT_NW(R)>(R.ord, true, w, alpha, c, c_per_share ? grp->eb : 0, n, r_out, host_threads(threads));
  });
  return MPVSS_OK;
}
extern "C" int mpvss_modp_group_poly_eval(const mpvss_modp_group* grp, const uint8_t* coeffs, size_t t, const int64_t* positions,
                                          size_t n, uint8_t* out, int threads) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  if (n == 0) return MPVSS_OK;
  if (!coeffs || !positions || !out || t == 0) return MPVSS_E_INVALID;
  for (size_t i = 0; i < n; ++i)
    if (positions[i] < 0) return MPVSS_E_INVALID;
  rt_rings(grp, [&](const auto& R) { poly_eval_bytes<RT_NW(R)>(R.ord, true, coeffs, t, positions, n, out, host_threads(threads)); });
  return MPVSS_OK;
}

namespace {

// The batch size from which the right-to-left twin kernel (shared squarings, 3 127 operations per share at 2048 bits, but a
// chain of that length) is taken instead of two left-to-right exponent sets in one launch (5 142 operations, chains of 2 571).
// Below it the chip is not full and the shorter chain wins.  Both paths give identical bytes.
// Measured per width, the same at 9 and 18 limbs per lane: profiles/modp_rt_deal_rate.txt (the tuning builds of
// `make twin-ab` pin it with -DMPVSS_RT_TWIN_MIN_SHARES=n).
#ifdef MPVSS_RT_TWIN_MIN_SHARES
size_t rt_twin_min_shares(int) { return (size_t)(MPVSS_RT_TWIN_MIN_SHARES); }
#else
size_t rt_twin_min_shares(int) { return 16384; }
#endif

// ---- the scalar ring Z/(q-1) on the device (DESIGN section 13, "Scalar ring on the device") -------------------------------------
// Mode 1 of mpvss_ctx_set_rt_scalar takes the device path from rt_scalar_min_shares shares of a whole call.  The threshold is what
// `tools/modp_rt_rate.py --scalar --ab` measures (profiles/modp_rt_scalar_rate.txt): the smallest n from which the whole call under
// mode 2 is no slower than the parent's at every larger measured n.  Until that is measured "automatic" means host, as
// RT_FD_AUTO_ON does for the forward differences.
size_t rt_scalar_min_shares(int) { return 16384; }   // UNMEASURED placeholder at every width
constexpr bool RT_SCALAR_AUTO_ON = false;

// THE launch decision of the scalar ring for one whole call of n shares (context lock held); counts the call
bool rt_scalar_on_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, size_t n) {
  const int mode = ctx->rt_scalar_mode;
  const bool dev = grp->has_q && n > 0 &&
                   (mode == 2 || (mode == 1 && RT_SCALAR_AUTO_ON && n >= rt_scalar_min_shares(grp->lpl)));
  ++(dev ? ctx->rt_scalar_dev_calls : ctx->rt_scalar_host_calls);
  return dev;
}

// ---- the per-share DLEQ hash on the device (DESIGN section 13, "Per-share hash on the device") ----------------------------------
// Mode 1 of mpvss_ctx_set_rt_share_hash takes the device path from rt_share_hash_min_shares shares of a whole call: the smallest
// measured n from which the whole call under mode 2 is no slower than the parent's at every larger measured n, from
// `tools/modp_rt_rate.py --share-hash --ab` (profiles/modp_rt_share_hash_rate.txt).  Measured at 1024, 2048 and 3072 bits: mode 2 is
// no slower at any measured n (1024, 4096, 65536; 16384 at 3072 bits), for both entry points, so the threshold is 1.
size_t rt_share_hash_min_shares(int) { return 1; }
constexpr bool RT_SHARE_HASH_AUTO_ON = true;

bool rt_share_hash_on_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, size_t n) {
  const int mode = ctx->rt_share_hash_mode;
  const bool dev = grp->has_sh && n > 0 &&
                   (mode == 2 || (mode == 1 && RT_SHARE_HASH_AUTO_ON && n >= rt_share_hash_min_shares(grp->lpl)));
  ++(dev ? ctx->rt_share_hash_dev_calls : ctx->rt_share_hash_host_calls);
  return dev;
}

// The dealer's coefficients for k_rt_modq_poly_eval: (a_j mod q') R mod q' as L limbs each, through pinned memory of the context
// into ctx->rt_sc_coef, and the parities of P at even (a_0) and odd (XOR of all a_j mod (q-1)) positions.  Both copies are the
// dealer's secret: `wipe` zeroes them whichever way the call ends.
int rt_stage_coeffs(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t, int* par_even, int* par_odd,
                    const uint32_t** coef_dev, RtWipe& wipe) {
  const size_t LW = rt_L(grp), EB = grp->eb, bytes = t * LW * 4;
  if (bytes > ctx->rt_sc_pin_cap) {
    if (ctx->rt_sc_pin) {
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      HIPCHK(ctx, hipHostFree(ctx->rt_sc_pin));
      ctx->rt_sc_pin = nullptr;
      ctx->rt_sc_pin_cap = 0;
    }
    const hipError_t e = hipHostMalloc(&ctx->rt_sc_pin, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
      ctx->rt_sc_pin = nullptr;
      return fail(ctx, MPVSS_E_NOMEM, "hipHostMalloc(coefficient staging)", e);
    }
    ctx->rt_sc_pin_cap = bytes;
  }
  wipe.pinned.push_back({ctx->rt_sc_pin, bytes});
  RET_IF(ensure(ctx, ctx->rt_sc_coef, bytes));
  wipe.device(ctx->rt_sc_coef, bytes);
  uint32_t* limbs = (uint32_t*)ctx->rt_sc_pin;
  *par_even = 0;
  *par_odd = 0;
  rt_rings(grp, [&](const auto& R) {
    constexpr int NW = RT_NW(R);
    uint64_t a[NW], r[NW], one_m[NW];
    hsc::from_bytes<NW>(one_m, grp->subR_be, true);
    for (size_t j = 0; j < t; ++j) {
      hsc::from_bytes<NW>(a, coeffs_host + j * EB, true);
      R.ord.reduce1(a);
      if (j == 0) *par_even = (int)(a[0] & 1);
      *par_odd ^= (int)(a[0] & 1);
      R.sub.mulmod(r, a, one_m);
      for (size_t k = 0; k < LW; ++k) {
        const size_t bit = 29 * k, w = bit / 64, sft = bit % 64;
        uint64_t v = w < (size_t)NW ? r[w] >> sft : 0;
        if (sft + 29 > 64 && w + 1 < (size_t)NW) v |= r[w + 1] << (64 - sft);
        limbs[j * LW + k] = (uint32_t)v & ((1u << 29) - 1);
      }
    }
    for (uint64_t* buf : {a, r}) {
      volatile uint64_t* wp = buf;
      for (int i = 0; i < NW; ++i) wp[i] = 0;
    }
  });
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_sc_coef.p, limbs, bytes, hipMemcpyHostToDevice, ctx->stream));
  *coef_dev = (const uint32_t*)ctx->rt_sc_coef.p;
  return 0;
}

// (-c) mod q' on the device (ctx->rt_sc_c) and c mod 2, for k_rt_modq_responses: c is reduced mod q - 1 first, which keeps its parity
int rt_stage_cneg(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* c_host, const uint8_t** cneg_dev, int* c_parity) {
  uint8_t neg[RT_EB_MAX];
  rt_rings(grp, [&](const auto& R) {
    constexpr int NW = RT_NW(R);
    uint64_t c[NW], m[NW];
    hsc::from_bytes<NW>(c, c_host, true);
    R.ord.reduce1(c);
    *c_parity = (int)(c[0] & 1);
    R.sub.reduce1(c);
    uint64_t o = 0;
    for (int i = 0; i < NW; ++i) o |= c[i];
    if (o) hsc::sub_n<NW>(m, R.sub.m, c); else memset(m, 0, sizeof(m));
    hsc::to_bytes<NW>(neg, m, true);
  });
  // the challenge is public; the staging buffer is a workspace of the context and the copy is drained before `neg` goes away
  RET_IF(ensure(ctx, ctx->rt_sc_c, grp->eb));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_sc_c.p, neg, grp->eb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *cneg_dev = (const uint8_t*)ctx->rt_sc_c.p;
  return 0;
}

const char* const RT_NO_Q = "no device scalar ring for this group: (q-1)/2 must be odd and >= 3 (mpvss_modp_group_has_device_scalar)";

// Shares per k_rt_twin_exp launch: 4096 waves, more than the chip holds at once, and it bounds the bucket scratch the context
// keeps at 2 x 15 x 65536 numbers (540 MiB at 18 limbs per lane, 270 MiB at 9, 150 MiB at 5) whatever MAX_CHUNK is.  At 27
// limbs per lane a share's buckets are 12 960 bytes: 32768 shares (2048 waves, 405 MiB) keep the same ceiling.  At 36 they
// are 17 280 bytes: 24576 shares (1536 waves) are the same 405 MiB.
size_t rt_twin_launch(int lpl) { return lpl == 36 ? 24576 : lpl == 27 ? 32768 : 65536; }

// out1 = B^e1, out2 = B^e2 for cnt shares (device pointers, one chunk).  Large batches: k_rt_twin_exp over bucket scratch of
// the context, of which the frame's wipe zeroes what the call used; small ones, two left-to-right exponent sets over the bases' tables
// in one launch.
int rt_twin_dev(RtCall& f, const uint8_t* bases, const uint8_t* e1, const uint8_t* e2, size_t cnt, uint8_t* out1, uint8_t* out2) {
  mpvss_ctx* const ctx = f.ctx;
  const mpvss_modp_group* const grp = f.grp;
  const modp_rt_consts* const dc = f.dc;
  const size_t EB = grp->eb, RT_TWIN_LAUNCH = rt_twin_launch(grp->lpl);
  if (cnt >= rt_twin_min_shares(grp->lpl)) {
    const size_t bytes = modp_rt_twin_scratch_bytes(grp->lpl, (int)std::min(cnt, RT_TWIN_LAUNCH));
    RET_IF(ensure(ctx, ctx->rt_buckets, bytes));
    f.wipe.device(ctx->rt_buckets, bytes);
    for (size_t off = 0; off < cnt; off += RT_TWIN_LAUNCH) {
      const size_t m = std::min(cnt - off, RT_TWIN_LAUNCH);
      TIMED_LAUNCH(ctx, 3, modp_rt_launch_twin_exp(grp->lpl, bases + off * EB, e1 + off * EB, e2 + off * EB, (int)m,
                                                   (uint32_t*)ctx->rt_buckets.p, out1 + off * EB, out2 + off * EB, dc, ctx->stream));
    }
    return 0;
  }
  const uint32_t* tb;
  RET_IF(rt_tables(ctx, grp, dc, bases, EB, cnt, ctx->rt_tab1, &tb));
  RET_IF(rt_exp_sets_any(ctx, grp, 3, tb, 16 * rt_L(grp), e1, e2, cnt, out1, out2, dc));
  return 0;
}

// out = base^e for one shared base (host bytes) and cnt exponents on the device: over the base's comb (rt_comb_for), or else
// left to right over its 16-entry table
int rt_fixed_base_dev(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, const uint8_t* base_host, const uint8_t* e,
                      size_t cnt, uint8_t* out, int timer) {
  const size_t EB = grp->eb;
  const uint32_t* comb;
  RET_IF(rt_comb_for(ctx, grp, dc, base_host, cnt, false, &comb));
  if (comb) {
    RET_IF(rt_comb_exp_any(ctx, grp, timer, comb, nullptr, 0, e, nullptr, 0, cnt, out, dc));
    return 0;
  }
  const uint8_t* db;
  RET_IF(rt_stage_small(ctx, grp, base_host, ctx->rt_small[0], &db));
  const uint32_t* tg;
  RET_IF(rt_tables(ctx, grp, dc, db, 0, 1, ctx->rt_tabg, &tg));
  RET_IF(rt_dual_exp_any(ctx, grp, timer, tg, 0, nullptr, 0, e, EB, nullptr, 0, cnt, out, dc));
  return 0;
}

bool rt_zero_mod_q(const mpvss_modp_group* grp, const uint8_t* v) {
  return rt_rings(grp, [&](const auto& R) {
    constexpr int NW = RT_NW(R);
    uint64_t x[NW];
    hsc::from_bytes<NW>(x, v, true);
    R.mod.reduce1(x);
    uint64_t o = 0;
    for (int i = 0; i < NW; ++i) o |= x[i];
    return o == 0;
  });
}

// The dealer's group side for n shares: X_i (commit_eval, or g^p_i when commitments is null: the dealer's own polynomial),
// Y_i = y_i^p_i and a2_i = y_i^w_i through the twin path, a1_i = g^w_i, and the transcript digest.  Outputs in `space`
// (the host ones optional).  p_values and witnesses are the frame's Secret inputs: zeroed where it staged them, and under
// f.secrets_dev device arrays of the caller whatever `space` says (group_deal's device-side scalar ring: P(i) never leaves HBM;
// the caller began the frame, launched into its spans already and wipes the two arrays itself).  The keys are the array
// `pubkeys`, or (pubkeys null) key_rows, the rows of a key set from the first share's key on: then both powers of a key are the two
// exponent sets of one k_rt_keyset_exp launch.
int rt_distribute_locked(RtCall& f, const uint8_t* commitments, size_t t, const int64_t* positions, const uint8_t* pubkeys,
                         const uint32_t* key_rows, const uint8_t* p_values, const uint8_t* witnesses, size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out,
                         uint8_t* a2_out, uint8_t* digest32_out) {
  mpvss_ctx* const ctx = f.ctx;
  const mpvss_modp_group* const grp = f.grp;
  mpvss::Sha256 h;
  std::vector<uint8_t> hv[4];                                   // X, Y, a1, a2 of one chunk for the transcript
  if (n > 0) {
    RET_IF(f.begin());
    if (commitments) RET_IF(rt_stage_commitments(f, commitments, t, n));
    RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
      const uint8_t* dy = pubkeys ? f.in(pubkeys, off, cnt, ctx->rt_in[1], RtCall::Public) : nullptr;
      const uint8_t* dp = f.in(p_values, off, cnt, ctx->rt_in[2], RtCall::Secret);
      const uint8_t* dw = f.in(witnesses, off, cnt, ctx->rt_in[3], RtCall::Secret);
      uint8_t* dX = f.out(x_out, off, cnt, ctx->rt_out[0]);
      uint8_t* d1 = f.out(a1_out, off, cnt, ctx->rt_out[1]);
      uint8_t* d2 = f.out(a2_out, off, cnt, ctx->rt_out[2]);
      uint8_t* dY = f.out(y_out, off, cnt, ctx->rt_out_y);
      RET_IF(f.rc);
      if (commitments) {
        const int64_t* dpos = f.in_positions(positions, off, cnt);
        RET_IF(f.rc);
        RET_IF(rt_commit_eval_dev(f, t, dpos, cnt, dX, positions + off));                             // participant.rs:207-215
      } else {
        RET_IF(rt_fixed_base_dev(ctx, grp, f.dc, grp->g_be, dp, cnt, dX, 0));                         // X_i = g^P(i)
      }
      RET_IF(rt_fixed_base_dev(ctx, grp, f.dc, grp->g_be, dw, cnt, d1, 1));                           // a1_i = g^w_i, dleq.rs:207-211
      // Y_i = y_i^P(i) (participant.rs:219), a2_i = y_i^w_i (dleq.rs:213-216): one base, two exponents
      if (pubkeys) {
        RET_IF(rt_twin_dev(f, dy, dp, dw, cnt, dY, d2));
      } else {
        TIMED_LAUNCH(ctx, 3, modp_rt_launch_keyset_exp(grp->lpl, key_rows + off * rt_keyset_stride(grp), nullptr, 0, dp, dw, nullptr, 0,
                                                       (int)cnt, dY, d2, f.dc, ctx->stream));
      }
      f.to_host(dX, cnt, hv[0]);
      f.to_host(dY, cnt, hv[1]);
      f.to_host(d1, cnt, hv[2]);
      f.to_host(d2, cnt, hv[3]);
      RET_IF(f.settle());
      frame_shares(h, hv[0].data(), hv[1].data(), hv[2].data(), hv[3].data(), 0, cnt, f.EB);          // participant.rs:238-245
      return 0;
    }));
    RET_IF(f.end());
  }
  uint8_t digest[32];
  h.final(digest);                                              // participant.rs:251
  if (digest32_out) memcpy(digest32_out, digest, 32);
  return MPVSS_OK;
}

// product of m elements (device bytes) by pairwise rounds through Montgomery form; result in buf[0..EB)
int rt_product_tree(mpvss_ctx* ctx, const mpvss_modp_group* grp, const modp_rt_consts* dc, uint8_t* buf, size_t m) {
  const size_t LW = rt_L(grp), EB = grp->eb;
  RET_IF(ensure(ctx, ctx->rt_tab1, m * LW * 4));
  uint32_t* lm = (uint32_t*)ctx->rt_tab1.p;
  while (m > 1) {
    const size_t half = m / 2;
    LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, buf, (int)(2 * half), lm, dc, ctx->stream));
    LAUNCHCHK(ctx, modp_rt_launch_mul(grp->lpl, lm, lm + half * LW, (int)half, buf, dc, ctx->stream));
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

extern "C" int mpvss_modp_group_twin_min_shares(const mpvss_modp_group* grp) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  return (int)std::min<size_t>(rt_twin_min_shares(grp->lpl), 0x7fffffff);
}

extern "C" int mpvss_modp_group_comb_min_shares(const mpvss_modp_group* grp) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  return (int)std::min<size_t>(rt_comb_min_shares(grp->lpl), 0x7fffffff);
}

extern "C" int mpvss_modp_group_comb_stats(mpvss_ctx* ctx, unsigned long long* builds, unsigned long long* hits,
                                           unsigned long long* evictions) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (builds) *builds = ctx->rt_comb_builds;
  if (hits) *hits = ctx->rt_comb_hits;
  if (evictions) *evictions = ctx->rt_comb_evictions;
  return MPVSS_OK;
}

extern "C" int mpvss_ctx_set_rt_fd(mpvss_ctx* ctx, int mode, int chains) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode < 0 || mode > 2 || chains < 0) return fail(ctx, MPVSS_E_INVALID, "set_rt_fd: mode is 0, 1 or 2 and chains >= 0");
  ctx->rt_fd_mode = mode;
  ctx->rt_fd_chains = chains;
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_fd_min_shares(const mpvss_modp_group* grp, size_t t) {
  if (rt_bad_group(grp) || t == 0) return MPVSS_E_INVALID;
  return (int)std::min<size_t>(rt_fd_min_shares(grp->lpl, t), 0x7fffffff);
}

extern "C" int mpvss_modp_group_fd_max_t(const mpvss_modp_group* grp) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  return modp_rt_fd_max_t(grp->lpl);
}

extern "C" int mpvss_modp_group_fd_stats(mpvss_ctx* ctx, unsigned long long* fd_calls, unsigned long long* horner_calls) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (fd_calls) *fd_calls = ctx->rt_fd_calls;
  if (horner_calls) *horner_calls = ctx->rt_horner_calls;
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_prepare(mpvss_ctx* ctx, const mpvss_modp_group* grp) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_prepare: no group");
  RtCall f(ctx, grp, MPVSS_HOST);
  RET_IF(f.begin());
  const uint32_t* comb;
  RET_IF(rt_comb_for(ctx, grp, f.dc, grp->g_be, 0, true, &comb));
  RET_IF(rt_comb_for(ctx, grp, f.dc, grp->G_be, 0, true, &comb));
  return f.end();
}

// generate_public_key (G^x) and the commitments C_j = g^a_j of a run-time group: one base for the whole call
extern "C" int mpvss_modp_group_batch_exp_fixed_base(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* base_host,
                                                     const uint8_t* exps, size_t n, uint8_t* out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_batch_exp_fixed_base: no group");
  if (n == 0) return MPVSS_OK;
  if (!base_host || !exps || !out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_batch_exp_fixed_base: bad argument");
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* de = f.in(exps, off, cnt, ctx->rt_in[2], RtCall::Secret);          // keygen secrets
    uint8_t* dout = f.out(out, off, cnt, ctx->rt_out[0]);
    RET_IF(f.rc);
    return rt_fixed_base_dev(ctx, grp, f.dc, base_host, de, cnt, dout, 1);
  }));
  return f.end();
}

extern "C" int mpvss_modp_group_batch_twin_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* bases,
                                               const uint8_t* e1, const uint8_t* e2, size_t n, uint8_t* out1, uint8_t* out2) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_batch_twin_exp: no group");
  if (n == 0) return MPVSS_OK;
  if (!bases || !e1 || !e2 || !out1 || !out2 || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_batch_twin_exp: bad argument");
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* db = f.in(bases, off, cnt, ctx->rt_in[0], RtCall::Public);
    const uint8_t* d1 = f.in(e1, off, cnt, ctx->rt_in[2], RtCall::Secret);
    const uint8_t* d2 = f.in(e2, off, cnt, ctx->rt_in[3], RtCall::Secret);
    uint8_t* o1 = f.out(out1, off, cnt, ctx->rt_out[0]);
    uint8_t* o2 = f.out(out2, off, cnt, ctx->rt_out[1]);
    RET_IF(f.rc);
    return rt_twin_dev(f, db, d1, d2, cnt, o1, o2);
  }));
  return f.end();
}

extern "C" int mpvss_modp_group_distribute(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments, size_t t,
                                           const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values,
                                           const uint8_t* witnesses, size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out,
                                           uint8_t* a2_out, uint8_t* digest32_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_distribute: no group");
  if (n > 0x7fffffff || (n > 0 && (!commitments || !positions || !pubkeys || !p_values || !witnesses || !x_out || !y_out || !a1_out ||
                                   !a2_out || t == 0 || t > 0x7fffffff)))
    return fail(ctx, MPVSS_E_INVALID, "group_distribute: bad argument");
  if (t > n) return fail(ctx, MPVSS_E_INVALID, "group_distribute: threshold > number of public keys (participant.rs:166)");
  RtCall f(ctx, grp, space);
  return rt_distribute_locked(f, commitments, t, positions, pubkeys, nullptr, p_values, witnesses, n, x_out, y_out, a1_out, a2_out, digest32_out);
}

namespace {
// group_deal with the scalar ring on the device (n > 0, arguments checked, context lock held).  Positions and witnesses are staged
// once for the whole call; k_rt_modq_poly_eval leaves P(i) in HBM, the group side reads P and w from there chunk by chunk, the
// challenge is hashed on the host as ever, and k_rt_modq_responses reads the same two arrays.  P and w of EVERY chunk must
// survive until the challenge is known, so the two buffers hold all n shares; with the responses' own array (r is copied back from
// it) the call holds 3 n EB bytes of HBM beside the chunk workspaces: 48 MiB for 65 536 shares of 256 bytes, 72 MiB of 384.  P
// and w join the frame's wipe, as do the staged coefficient limbs.  Same bytes as the host path.
int rt_deal_scalar_dev(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                       const uint8_t* pubkeys_host, const uint32_t* key_rows, const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out,
                       uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out256, uint8_t* r_out) {
  const size_t EB = grp->eb;
  RtCall f(ctx, grp, MPVSS_HOST);
  f.secrets_dev = true;
  RET_IF(f.begin(RtCall::SubQ));
  int par_even, par_odd;
  const uint32_t* coef;
  RET_IF(rt_stage_coeffs(ctx, grp, coeffs_host, t, &par_even, &par_odd, &coef, f.wipe));
  uint8_t* dP = f.work(ctx->rt_sc_p, n, RtCall::Secret);
  uint8_t* dW = f.work(ctx->rt_sc_w, n, RtCall::Secret);
  RET_IF(f.rc);
  const void* dpos;
  RET_IF(stage_in(ctx, MPVSS_HOST, positions_host, n * 8, ctx->w->pos, &dpos));
  HIPCHK(ctx, hipMemcpyAsync(dW, witnesses_host, n * EB, hipMemcpyHostToDevice, ctx->stream));
  TIMED_LAUNCH(ctx, 4, modp_rt_launch_modq_poly_eval(grp->lpl, coef, (int)t, (const int64_t*)dpos, (int)n, par_even, par_odd, dP, f.dcq,
                                                     ctx->stream));                                      // participant.rs:202
  uint8_t digest[32], challenge[RT_EB_MAX];
  RET_IF(rt_distribute_locked(f, nullptr, t, positions_host, pubkeys_host, key_rows, dP, dW, n, x_out, y_out, a1_out, a2_out, digest));
  rt_hash_to_scalar(grp, digest, 32, challenge);                 // participant.rs:251-252
  if (digest32_out) memcpy(digest32_out, digest, 32);
  if (challenge_out256) memcpy(challenge_out256, challenge, EB);
  const uint8_t* dcneg;
  int c_parity;
  RET_IF(rt_stage_cneg(ctx, grp, challenge, &dcneg, &c_parity));
  uint8_t* dR = f.work(ctx->rt_sc_r, n);
  RET_IF(f.rc);
  TIMED_LAUNCH(ctx, 4, modp_rt_launch_modq_responses(grp->lpl, dW, dP, dcneg, c_parity, (int)n, dR, f.dcq, ctx->stream));   // :255-264
  HIPCHK(ctx, hipMemcpyAsync(r_out, dR, n * EB, hipMemcpyDeviceToHost, ctx->stream));
  return f.end();
}
}  // namespace

// participant.rs:160-286 after "draw the polynomial and the witnesses": P(i) mod (q-1), the group side above with X_i = g^P(i), the
// challenge and the responses r_i = w_i - P(i) c.  The scalar ring runs on the device (rt_deal_scalar_dev) when
// mpvss_ctx_set_rt_scalar and the handle allow it, otherwise on host threads.  Arguments checked, context lock held; the keys are
// pubkeys_host, or (pubkeys_host null) key_rows of a key set.
namespace {
int rt_deal_locked(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                   const uint8_t* pubkeys_host, const uint32_t* key_rows, const uint8_t* witnesses_host, size_t n, uint8_t* x_out,
                   uint8_t* y_out, uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out256, uint8_t* r_out) {
  const size_t EB = grp->eb;
  RET_IF(check_positions_host(ctx, positions_host, n));
  if (rt_scalar_on_device(ctx, grp, n))
    return rt_deal_scalar_dev(ctx, grp, coeffs_host, t, positions_host, pubkeys_host, key_rows, witnesses_host, n, x_out, y_out, a1_out,
                              a2_out, digest32_out, challenge_out256, r_out);
  std::vector<uint8_t> P(n * EB);
  RtCall f(ctx, grp, MPVSS_HOST);
  f.wipe.host.push_back(&P);
  const int threads = host_threads(0);
  if (n > 0)                                                                                               // participant.rs:202
    rt_rings(grp, [&](const auto& R) { poly_eval_bytes<RT_NW(R)>(R.ord, true, coeffs_host, t, positions_host, n, P.data(), threads); });
  uint8_t digest[32], challenge[RT_EB_MAX];
  RET_IF(rt_distribute_locked(f, nullptr, t, positions_host, pubkeys_host, key_rows, P.data(), witnesses_host, n, x_out, y_out, a1_out,
                              a2_out, digest));
  rt_hash_to_scalar(grp, digest, 32, challenge);                 // participant.rs:251-252
  if (digest32_out) memcpy(digest32_out, digest, 32);
  if (challenge_out256) memcpy(challenge_out256, challenge, EB);
  if (n > 0)                                                                                               // :255-264
    rt_rings(grp, [&](const auto& R) { responses_bytes<RT_NW(R)>(R.ord, true, witnesses_host, P.data(), challenge, 0, n, r_out, threads); });
  return MPVSS_OK;
}
}  // namespace

extern "C" int mpvss_modp_group_deal(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t,
                                     const int64_t* positions_host, const uint8_t* pubkeys_host, const uint8_t* witnesses_host, size_t n,
                                     uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out,
                                     uint8_t* challenge_out256, uint8_t* r_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_deal: no group");
  if (n > 0x7fffffff || t > 0x7fffffff ||
      (n > 0 && (!coeffs_host || !positions_host || !pubkeys_host || !witnesses_host || !y_out || !r_out || t == 0)))
    return fail(ctx, MPVSS_E_INVALID, "group_deal: bad argument (t >= 1, n < 2^31)");
  if (t > n) return fail(ctx, MPVSS_E_INVALID, "group_deal: threshold > number of public keys (participant.rs:166)");
  return rt_deal_locked(ctx, grp, coeffs_host, t, positions_host, pubkeys_host, nullptr, witnesses_host, n, x_out, y_out, a1_out, a2_out,
                        digest32_out, challenge_out256, r_out);
}

// participant.rs:294-353 for n participants: S_i = Y_i^(1/x_i), a1_i = G^w_i, a2_i = S_i^w_i = Y_i^(w_i / x_i) -- S and a2 share
// the base Y_i, so with e2_i = w_i xinv_i mod (q-1) (host threads) both come from the twin path.  That is exact for a unit
// Y_i; a Y_i that is 0 mod q makes S_i = 0 and a2_i = 0^w_i (modp.rs:122-128), where the reduced exponent would matter: a
// chunk that holds such a row runs the two dependent k_rt_dual_exp chains instead.
extern "C" int mpvss_modp_group_extract_shares(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* pk,
                                               const uint8_t* y, const uint8_t* xinv, const uint8_t* w, size_t n, uint8_t* s_out,
                                               uint8_t* c_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_extract_shares: no group");
  const size_t EB = grp->eb;
  if (n == 0) return MPVSS_OK;
  if (!pk || !y || !xinv || !w || !s_out || !c_out_host || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_extract_shares: bad argument");
  std::vector<uint8_t> hpk, hy, hxi, hw, e2, hS, h1, h2, c32;
  RtCall f(ctx, grp, space);
  f.wipe.host.push_back(&e2);
  const int threads = host_threads(0);
  // e2 = w / x on the device (k_rt_modq_mul from the staged w and xinv) or on host threads; the zero-row scan of Y stays here
  const bool sdev = rt_scalar_on_device(ctx, grp, n);
  // the challenges from k_rt_share_verdict (a1 and a2 never leave the device) or framed and hashed on host threads
  const bool hdev = rt_share_hash_on_device(ctx, grp, n);
  RET_IF(f.begin(sdev ? RtCall::ModQ | RtCall::SubQ : RtCall::ModQ));
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* PK = hdev ? nullptr : f.host_view(pk, off, cnt, hpk);
    const uint8_t* Y = f.host_view(y, off, cnt, hy);
    const uint8_t* XI = sdev ? nullptr : f.host_view(xinv, off, cnt, hxi, RtCall::Secret);
    const uint8_t* W = sdev ? nullptr : f.host_view(w, off, cnt, hw, RtCall::Secret);
    RET_IF(f.host_ready());
    if (!sdev) e2.resize(cnt * EB);
    std::atomic<int> zero_row{0};
    hsc::parallel_for(cnt, threads, [&](size_t lo, size_t hi) {
      bool z = false;
      for (size_t i = lo; i < hi; ++i) {
        if (!sdev)
          rt_rings(grp, [&](const auto& R) { scalar_mul_bytes<RT_NW(R)>(R.ord, true, W + i * EB, XI + i * EB, e2.data() + i * EB); });
        z = z || rt_zero_mod_q(grp, Y + i * EB);
      }
      if (z) zero_row.store(1);
    });
    const bool shared = zero_row.load() == 0;
    const uint8_t* dy = f.in(y, off, cnt, ctx->rt_in[0], RtCall::Public);
    const uint8_t* dxi = f.in(xinv, off, cnt, ctx->rt_in[1], RtCall::Secret);
    const uint8_t* dw = f.in(w, off, cnt, ctx->rt_in[3], RtCall::Secret);
    // e2 lives in rt_in[2] wherever it was formed: a secret of the library's own making, zeroed in either space
    const uint8_t* de2 = sdev ? f.work(ctx->rt_in[2], cnt, RtCall::Secret) : f.in_host(e2.data(), cnt, ctx->rt_in[2], RtCall::Secret);
    uint8_t* dS = f.out(s_out, off, cnt, ctx->rt_out[0]);
    uint8_t* d1 = f.work(ctx->rt_out[1], cnt);
    uint8_t* d2 = f.work(ctx->rt_out[2], cnt);
    const uint8_t* dpk = hdev ? f.in(pk, off, cnt, ctx->rt_in[5], RtCall::Public) : nullptr;
    uint8_t* dc32 = hdev ? f.raw(ctx->rt_sh_c32, cnt * 32) : nullptr;
    RET_IF(f.rc);
    if (sdev && shared)                                          // a chunk with a zero row takes the two dependent chains: no e2
      TIMED_LAUNCH(ctx, 4, modp_rt_launch_modq_mul(grp->lpl, dw, dxi, (int)cnt, (uint8_t*)de2, f.dcq, ctx->stream));
    if (shared) {
      RET_IF(rt_twin_dev(f, dy, dxi, de2, cnt, dS, d2));
    } else {
      const uint32_t* tb;
      RET_IF(rt_tables(ctx, grp, f.dc, dy, EB, cnt, ctx->rt_tab1, &tb));                               // S = Y^(1/x), :310-314
      RET_IF(rt_dual_exp_any(ctx, grp, 3, tb, 16 * rt_L(grp), nullptr, 0, dxi, EB, nullptr, 0, cnt, dS, f.dc));
      RET_IF(rt_tables(ctx, grp, f.dc, dS, EB, cnt, ctx->rt_tab2, &tb));                               // a2 = S^w
      RET_IF(rt_dual_exp_any(ctx, grp, 3, tb, 16 * rt_L(grp), nullptr, 0, dw, EB, nullptr, 0, cnt, d2, f.dc));
    }
    RET_IF(rt_fixed_base_dev(ctx, grp, f.dc, grp->G_be, dw, cnt, d1, 1));                              // a1 = G^w
    if (hdev) {                                                  // :329-343; S goes out by settle(), the challenges as 32 bytes each
      RET_IF(rt_share_hash_dev(f, dpk, dy, d1, d2, nullptr, cnt, nullptr, dc32, 32));
      c32.resize(cnt * 32);
      f.host_bytes(c32.data(), dc32, cnt * 32);
      RET_IF(f.settle());
      rt_widen_challenges(c32.data(), cnt, EB, c_out_host + off * EB);
      return 0;
    }
    f.to_host(dS, cnt, hS);
    f.to_host(d1, cnt, h1);
    f.to_host(d2, cnt, h2);
    RET_IF(f.settle());
    hsc::parallel_for(cnt, threads, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i)                                                                // :329-343
        rt_share_challenge(grp, PK + i * EB, Y + i * EB, h1.data() + i * EB, h2.data() + i * EB, c_out_host + (off + i) * EB);
    });
    return 0;
  }));
  return f.end();
}

namespace {

// lambda_i of a position list as the exponent of S_i: |lambda_i| mod (q-1)/2 in lowest terms (lagrange_coefficient_at_zero), and
// (q-1) - |lambda_i| for a negative coefficient of nonzero magnitude.  *neg: the sign, which the zero-share check needs.  False:
// duplicate positions, or a denominator that has no inverse even in lowest terms.
bool rt_lagrange_exponent(const mpvss_modp_group* grp, const int64_t* positions, size_t m, size_t i, uint8_t* exp_out, char* neg) {
  return rt_rings(grp, [&](const auto& R) {
    constexpr int NW = RT_NW(R);
    uint64_t e[NW];
    if (!lagrange_coefficient_at_zero<NW>(R.sub, positions, m, i, e, neg)) return false;
    if (*neg) {
      uint64_t o = 0;
      for (int k = 0; k < NW; ++k) o |= e[k];
      if (o) hsc::sub_n<NW>(e, R.ord.m, e);
    }
    hsc::to_bytes<NW>(exp_out, e, true);
    return true;
  });
}

// ---- the same exponents on the device (DESIGN section 13, "Lagrange exponents on the device") -----------------------------------
// A list longer than this keeps the host path: at these widths a launch at the curve groups' 2^20 would run for minutes.  Nobody
// has measured above it.
constexpr size_t RT_LAGRANGE_DEVICE_MAX_M = 16384;
// Mode 1 of mpvss_ctx_set_rt_lagrange takes the device for a call whose work -- the sum of m^2 over its distinct position lists,
// m^2 of a lone secret -- is at least this: the smallest measured work from which, at every measured shape at or above it and at
// every measured width, the median of mode 2 lies below the minimum of mode 0 (tools/modp_rt_reconstruct_many.py --lagrange against
// a build of the parent commit, fresh processes, profiles/modp_rt_lagrange_device.txt).  At 1024 and 2048 bits that is 60 secrets
// of 32 shares with a list each, 60 x 32^2 (6.6 against 12.3 ms, 31.5 against 31.8 ms); every measured shape above it is faster on
// the device (60 x 1024 with a list each 25 against 814 ms and 119 against 1 499 ms, one secret of 16 384 shares 89 ms against
// 3.6 s), the four below it -- 9, 1 024, 1 156 and 3 600 -- are slower by the latency of one Fermat power, 3 and 15 ms.  At 3072
// and 4096 bits only 60 x 1024 with a list each is measured (346 ms against 2.9 s, 892 ms against 4.6 s): automatic starts there.
// Nothing between 3 600 and 61 440 is measured, nor anything below 1024 bits: automatic stays on the host below the figure.
double rt_lagrange_min_work(int lpl) { return lpl > 18 ? 60.0 * 1024 * 1024 : 60.0 * 32 * 32; }

// THE launch decision of the Lagrange exponents: `work` as above, the longest list and the coefficients of the call
bool rt_lagrange_on_device(const mpvss_ctx* ctx, const mpvss_modp_group* grp, double work, size_t longest, size_t coefs) {
  // (tile rows hold positions' and coefficients' indices in 32 bits)
  if (ctx->rt_lagrange_mode == 0 || !grp->has_q || longest > RT_LAGRANGE_DEVICE_MAX_M || coefs >= 0x80000000u) return false;
  return ctx->rt_lagrange_mode == 2 || work >= rt_lagrange_min_work(grp->lpl);
}

// The signs of a list's coefficients: lambda_i is negative for an odd number of positions below x_i, the parity of the rank of x_i
// in the sorted list.  False: duplicate positions (what the quadratic host loop finds on its way).
bool rt_lagrange_signs(const int64_t* pos, size_t m, char* neg) {
  std::vector<std::pair<int64_t, size_t>> s(m);
  for (size_t i = 0; i < m; ++i) s[i] = {pos[i], i};
  std::sort(s.begin(), s.end());
  for (size_t r = 0; r + 1 < m; ++r)
    if (s[r].first == s[r + 1].first) return false;
  for (size_t r = 0; r < m; ++r) neg[s[r].second] = (char)(r & 1);
  return true;
}

constexpr size_t RT_LAGRANGE_TILE = 16;            // RT_NUMS of modp_rt_kernels.inc: coefficients of a tile, slots of a workgroup

// a list of a launch: where it starts in the launch's positions (and coefficients), its length, its positions
struct RtLagrangeList {
  size_t first, m;
  const int64_t* pos;
};

// The exponents of the admitted lists `lists` (positions >= 1 and pairwise different, signs in negs) of a launch whose `total`
// positions lie back to back in all_pos: exps_dev[c] (EB bytes) for coefficient c = position c.  The frame has begun with the
// constants of q'.  Tiles travel in chunks of at most MAX_CHUNK slots, 16 per tile, over the context's workspaces: numerators and
// denominators in rt_tab1, the denominators' bytes and inverses in rt_out[1] and rt_out[2], their tables in rt_tab2 --
// k_rt_lagrange_terms, k_rt_table, k_rt_dual_exp with q' - 2 at stride 0, k_rt_lagrange_finish, all timed as kind 4.  A list with
// a failed flag (a denominator without Fermat inverse: 0 mod a small q', or a composite q') is recomputed WHOLE by
// rt_lagrange_exponent, which decides between a value and a refusal (list_ok[l] = 0); its exponents are uploaded into its slice.
// Counts the lists.  Synchronous: the stream is drained on every way out, so all_pos and negs need not outlive the call.
int rt_lagrange_dev(RtCall& f, DevBuf& pos_buf, DevBuf& tile_buf, DevBuf& neg_buf, const int64_t* all_pos, const char* negs, size_t total,
                    const std::vector<RtLagrangeList>& lists, uint8_t* exps_dev, std::vector<char>& list_ok) {
  mpvss_ctx* ctx = f.ctx;
  const mpvss_modp_group* grp = f.grp;
  const size_t EB = grp->eb, L = rt_L(grp);
  std::vector<uint32_t> tiles;
  std::vector<uint8_t> flags(total, 1), redo;
  StreamDrain drain{ctx};
  for (const RtLagrangeList& l : lists)
    for (size_t off = 0; off < l.m; off += RT_LAGRANGE_TILE) {
      const uint32_t row[4] = {(uint32_t)l.first, (uint32_t)l.m, (uint32_t)(l.first + off), (uint32_t)std::min(l.m - off, RT_LAGRANGE_TILE)};
      tiles.insert(tiles.end(), row, row + 4);
    }
  const size_t ntiles = tiles.size() / 4;
  if (ntiles == 0) return MPVSS_OK;
  const size_t chunk_tiles = std::min(ntiles, std::max<size_t>(MAX_CHUNK / RT_LAGRANGE_TILE, 1)), slots = chunk_tiles * RT_LAGRANGE_TILE;
  RET_IF(ensure(ctx, pos_buf, total * 8));
  RET_IF(ensure(ctx, tile_buf, tiles.size() * 4));
  RET_IF(ensure(ctx, neg_buf, total));
  RET_IF(ensure(ctx, ctx->rt_lag_flags, total));
  RET_IF(ensure(ctx, ctx->rt_lag_e, EB));
  RET_IF(ensure(ctx, ctx->rt_tab1, 2 * slots * L * 4));
  RET_IF(ensure(ctx, ctx->rt_tab2, slots * 16 * L * 4));
  RET_IF(ensure(ctx, ctx->rt_out[1], slots * EB));
  RET_IF(ensure(ctx, ctx->rt_out[2], slots * EB));
  HIPCHK(ctx, hipMemcpyAsync(pos_buf.p, all_pos, total * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(tile_buf.p, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(neg_buf.p, negs, total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_lag_e.p, grp->subm2_be, EB, hipMemcpyHostToDevice, ctx->stream));
  uint32_t* num_m = (uint32_t*)ctx->rt_tab1.p;
  uint32_t* den_m = num_m + slots * L;
  uint32_t* tab = (uint32_t*)ctx->rt_tab2.p;
  uint8_t* den_be = (uint8_t*)ctx->rt_out[1].p;
  uint8_t* dinv_be = (uint8_t*)ctx->rt_out[2].p;
  for (size_t t0 = 0; t0 < ntiles; t0 += chunk_tiles) {
    const int nt = (int)std::min(chunk_tiles, ntiles - t0), ns = nt * (int)RT_LAGRANGE_TILE;
    const uint32_t* rows = (const uint32_t*)tile_buf.p + 4 * t0;
    TIMED_LAUNCH(ctx, 4, modp_rt_launch_lagrange_terms(grp->lpl, (const int64_t*)pos_buf.p, rows, nt, num_m, den_m, den_be, f.dcq, ctx->stream));
    TIMED_LAUNCH(ctx, 4, modp_rt_launch_table(grp->lpl, den_be, EB, ns, tab, f.dcq, ctx->stream));
    RET_IF(rt_dual_exp_any(ctx, grp, 4, tab, 16 * L, nullptr, 0, (const uint8_t*)ctx->rt_lag_e.p, 0, nullptr, 0, ns, dinv_be, f.dcq));   // den^(q'-2)
    TIMED_LAUNCH(ctx, 4, modp_rt_launch_lagrange_finish(grp->lpl, rows, nt, num_m, den_m, dinv_be, (const uint8_t*)neg_buf.p, exps_dev,
                                                        (uint8_t*)ctx->rt_lag_flags.p, f.dcq, ctx->stream));
  }
  for (const RtLagrangeList& l : lists)                  // (only the slices of the launch's lists were written)
    HIPCHK(ctx, hipMemcpyAsync(flags.data() + l.first, (const uint8_t*)ctx->rt_lag_flags.p + l.first, l.m, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < lists.size(); ++k) {
    const RtLagrangeList& l = lists[k];
    const uint8_t* fl = flags.data() + l.first;
    if (std::find(fl, fl + l.m, 0) == fl + l.m) {
      ++ctx->rt_lagrange_dev_lists;
      continue;
    }
    redo.resize(l.m * EB);
    char sign;
    bool ok = true;
    for (size_t i = 0; i < l.m && ok; ++i) ok = rt_lagrange_exponent(grp, l.pos, l.m, i, redo.data() + i * EB, &sign);
    list_ok[k] = ok ? 1 : 0;
    if (!ok) continue;
    HIPCHK(ctx, hipMemcpyAsync(exps_dev + l.first * EB, redo.data(), l.m * EB, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // (redo is filled again by the next such list)
    ++ctx->rt_lagrange_fallback_lists;
    ++ctx->rt_lagrange_host_lists;
  }
  return MPVSS_OK;
}

const char* const RT_NO_LAGRANGE = "group_reconstruct: duplicate positions, or a Lagrange coefficient whose denominator in lowest terms has no inverse mod (q-1)/2";

// the m exponents and signs of one list computed here, on the host (into exps_own) or on the device (into rt_in[1], which
// k_rt_dual_exp reads its exponents from: *exps_dev)
int rt_lagrange_one(RtCall& f, const int64_t* positions_host, size_t m, std::vector<uint8_t>& exps_own, std::vector<char>& neg_own,
                    const uint8_t** exps_dev) {
  mpvss_ctx* ctx = f.ctx;
  const size_t EB = f.grp->eb;
  neg_own.assign(m, 0);
  if (rt_lagrange_on_device(ctx, f.grp, (double)m * (double)m, m, m)) {
    if (!rt_lagrange_signs(positions_host, m, neg_own.data())) return fail(ctx, MPVSS_E_INVALID, RT_NO_LAGRANGE);
    RET_IF(f.begin(RtCall::SubQ));
    uint8_t* dE = f.work(ctx->rt_in[1], m);
    RET_IF(f.rc);
    std::vector<char> list_ok(1, 1);
    RET_IF(rt_lagrange_dev(f, ctx->rt_lag_pos, ctx->rt_lag_tiles, ctx->rt_lag_neg, positions_host, neg_own.data(), m,
                           {RtLagrangeList{0, m, positions_host}}, dE, list_ok));
    if (!list_ok[0]) return fail(ctx, MPVSS_E_INVALID, RT_NO_LAGRANGE);
    *exps_dev = dE;
    return MPVSS_OK;
  }
  exps_own.resize(m * EB);
  for (size_t i = 0; i < m; ++i)
    if (!rt_lagrange_exponent(f.grp, positions_host, m, i, exps_own.data() + i * EB, &neg_own[i])) return fail(ctx, MPVSS_E_INVALID, RT_NO_LAGRANGE);
  ++ctx->rt_lagrange_host_lists;
  return MPVSS_OK;
}

// int_BE(SHA256(element_to_bytes(G^s))) mod q (participant.rs:512-515): the reduction matters for q below 2^256
void rt_secret_mask(const mpvss_modp_group* grp, const uint8_t* gs, uint8_t* mask_out32) {
  const size_t EB = grp->eb;
  uint8_t hb[RT_EB_MAX];
  memset(hb, 0, EB - 32);
  mpvss::Sha256 h;
  frame_min_bytes_update(h, gs, EB);
  h.final(hb + EB - 32);
  rt_rings(grp, [&](const auto& R) {
    constexpr int NW = RT_NW(R);
    uint64_t x[NW];
    hsc::from_bytes<NW>(x, hb, true);
    R.mod.reduce1(x);
    hsc::to_bytes<NW>(hb, x, true);
  });
  memcpy(mask_out32, hb + EB - 32, 32);
}

// participant.rs:462-561: G^s = prod_i S_i^lambda_i.  Lagrange exponents mod (q-1)/2 with the sign kept aside (:526-561); a
// negative coefficient inverts the factor, and S^-e = S^((q-1) - e) for every unit S mod a prime q, so the m powers run in one
// k_rt_dual_exp launch with no inversion at all.  (q-1)/2 must be odd (every safe prime above 5).  A coefficient is reduced to
// lowest terms before its denominator is inverted (:546-553), which matters only for a (q-1)/2 small enough to divide a position
// or a difference of two: lagrange_at_zero does so where the raw denominator has no inverse.
// The body of mpvss_modp_group_reconstruct (context lock held, the group checked).  exps_pre / neg_pre: the m exponents and signs
// when the caller has them already (mpvss_modp_group_reconstruct_many computed them with the call's other position lists), the
// exponents in host memory (exps_pre) or in device memory (exps_dev); else they are computed here, on the host or on the device.
int rt_reconstruct_locked(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const int64_t* positions_host, const uint8_t* shares,
                          size_t m, uint8_t* gs_out256, uint8_t* mask_out32, const uint8_t* exps_pre, const char* neg_pre,
                          const uint8_t* exps_dev = nullptr) {
  const size_t EB = grp->eb;
  if (!positions_host || !shares || m == 0 || !gs_out256 || m > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_reconstruct: bad argument");
  for (size_t i = 0; i < m; ++i)
    if (positions_host[i] < 1) return fail(ctx, MPVSS_E_INVALID, "group_reconstruct: positions must be >= 1 (util.rs:47-64)");
  std::vector<char> neg_own;
  std::vector<uint8_t> exps_own, hs;
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  if (!exps_pre && !exps_dev) RET_IF(rt_lagrange_one(f, positions_host, m, exps_own, neg_own, &exps_dev));
  const uint8_t* exps = exps_pre ? exps_pre : exps_own.data();
  const char* neg = neg_pre ? neg_pre : neg_own.data();
  // a share that is 0 mod q has no inverse: the reference returns None when its coefficient is negative (:551-553)
  const uint8_t* S = f.host_view(shares, 0, m, hs);
  RET_IF(f.host_ready());
  for (size_t i = 0; i < m; ++i)
    if (neg[i] && rt_zero_mod_q(grp, S + i * EB))
      return fail(ctx, MPVSS_E_INVALID, "group_reconstruct: a share is 0 mod q and has no inverse");
  const uint8_t* dS = f.in(shares, 0, m, ctx->rt_in[0], RtCall::Public);
  const uint8_t* dE = exps_dev ? exps_dev : f.in_host(exps, m, ctx->rt_in[1], RtCall::Public);
  uint8_t* dF = f.work(ctx->rt_out[0], m);
  RET_IF(f.rc);
  const uint32_t* tb;
  RET_IF(rt_tables(ctx, grp, f.dc, dS, EB, m, ctx->rt_tab2, &tb));
  RET_IF(rt_dual_exp_any(ctx, grp, 3, tb, 16 * rt_L(grp), nullptr, 0, dE, EB, nullptr, 0, m, dF, f.dc));   // S_i^lambda_i
  RET_IF(rt_product_tree(ctx, grp, f.dc, dF, m));                                                      // fold with mul, :503-505
  std::vector<uint8_t> gs;
  f.to_host(dF, 1, gs);
  RET_IF(f.settle());
  memcpy(gs_out256, gs.data(), EB);
  if (mask_out32) rt_secret_mask(grp, gs.data(), mask_out32);
  return f.end();
}

}  // namespace

extern "C" int mpvss_modp_group_reconstruct(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const int64_t* positions_host,
                                            const uint8_t* shares, size_t m, uint8_t* gs_out256, uint8_t* mask_out32) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_reconstruct: no group");
  return rt_reconstruct_locked(ctx, grp, space, positions_host, shares, m, gs_out256, mask_out32, nullptr, nullptr);
}

// =====================================================================================================================
// The scalar ring Z/(q-1) of a run-time group on the device: the handle's counterparts of mpvss_modp_poly_eval_device and
// mpvss_modp_dleq_responses_device, and the ring's product per share.  They need the constants of q' (has_q) and have no host
// path of their own: a handle without them is MPVSS_E_INVALID.  On ctx->stream under the context lock.
// =====================================================================================================================
extern "C" int mpvss_modp_group_has_device_scalar(const mpvss_modp_group* grp) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  return grp->has_q ? 1 : 0;
}

extern "C" int mpvss_ctx_set_rt_scalar(mpvss_ctx* ctx, int mode) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode < 0 || mode > 2) return fail(ctx, MPVSS_E_INVALID, "set_rt_scalar: mode is 0, 1 or 2");
  ctx->rt_scalar_mode = mode;
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_scalar_stats(mpvss_ctx* ctx, unsigned long long* device_calls, unsigned long long* host_calls) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (device_calls) *device_calls = ctx->rt_scalar_dev_calls;
  if (host_calls) *host_calls = ctx->rt_scalar_host_calls;
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_scalar_min_shares(const mpvss_modp_group* grp) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  return (int)std::min<size_t>(rt_scalar_min_shares(grp->lpl), 0x7fffffff);
}

extern "C" int mpvss_modp_group_poly_eval_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t,
                                                 const int64_t* positions_dev, size_t n, uint8_t* out_dev) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_poly_eval_device: no group");
  if (n == 0) return MPVSS_OK;
  if (!coeffs_host || !positions_dev || !out_dev || t == 0 || t > 0x7fffffff || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_poly_eval_device: bad argument (t must be >= 1)");
  if (!grp->has_q) return fail(ctx, MPVSS_E_INVALID, RT_NO_Q);
  std::vector<int64_t> hp(n);          // declared before the frame, which drains the copy into it before it goes away
  RtCall f(ctx, grp, MPVSS_DEVICE);
  RET_IF(f.begin(RtCall::SubQ));
  int par_even, par_odd;
  const uint32_t* coef;
  RET_IF(rt_stage_coeffs(ctx, grp, coeffs_host, t, &par_even, &par_odd, &coef, f.wipe));
  TIMED_LAUNCH(ctx, 4, modp_rt_launch_modq_poly_eval(grp->lpl, coef, (int)t, positions_dev, (int)n, par_even, par_odd, out_dev, f.dcq,
                                                     ctx->stream));
  // positions are validated after the fact, as mpvss_modp_poly_eval_device does (a negative one is the caller's bug)
  HIPCHK(ctx, hipMemcpyAsync(hp.data(), positions_dev, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  RET_IF(f.end());
  for (size_t i = 0; i < n; ++i)
    if (hp[i] < 0) return fail(ctx, MPVSS_E_INVALID, "negative position (the reference panics: negative exponent)");
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_dleq_responses_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* w_dev,
                                                      const uint8_t* alpha_dev, const uint8_t* c_host, size_t n, uint8_t* r_dev_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_dleq_responses_device: no group");
  if (n == 0) return MPVSS_OK;
  if (!w_dev || !alpha_dev || !c_host || !r_dev_out || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "group_dleq_responses_device: bad argument");
  if (!grp->has_q) return fail(ctx, MPVSS_E_INVALID, RT_NO_Q);
  RtCall f(ctx, grp, MPVSS_DEVICE);
  RET_IF(f.begin(RtCall::SubQ));
  const uint8_t* dcneg;
  int c_parity;
  RET_IF(rt_stage_cneg(ctx, grp, c_host, &dcneg, &c_parity));
  TIMED_LAUNCH(ctx, 4, modp_rt_launch_modq_responses(grp->lpl, w_dev, alpha_dev, dcneg, c_parity, (int)n, r_dev_out, f.dcq, ctx->stream));
  return f.end();
}

extern "C" int mpvss_modp_group_batch_scalar_mul(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* a,
                                                 const uint8_t* b, size_t n, uint8_t* out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_batch_scalar_mul: no group");
  if (n == 0) return MPVSS_OK;
  if (!a || !b || !out || n > 0x7fffffff || (space != MPVSS_HOST && space != MPVSS_DEVICE))
    return fail(ctx, MPVSS_E_INVALID, "group_batch_scalar_mul: bad argument");
  if (!grp->has_q) return fail(ctx, MPVSS_E_INVALID, RT_NO_Q);
  RtCall f(ctx, grp, space);
  RET_IF(f.begin(RtCall::SubQ));
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {      // scalars of the ring are secrets wherever the protocol forms products
    const uint8_t* da = f.in(a, off, cnt, ctx->rt_in[2], RtCall::Secret);
    const uint8_t* db = f.in(b, off, cnt, ctx->rt_in[3], RtCall::Secret);
    uint8_t* dout = f.out(out, off, cnt, ctx->rt_out[0], RtCall::Secret);
    RET_IF(f.rc);
    TIMED_LAUNCH(ctx, 4, modp_rt_launch_modq_mul(grp->lpl, da, db, (int)cnt, dout, f.dcq, ctx->stream));
    return 0;
  }));
  return f.end();
}

// =====================================================================================================================
// The per-share DLEQ hash of a run-time group on the device (DESIGN section 13, "Per-share hash on the device"): where
// group_verify_shares / group_extract_shares hash, and the challenges of n transcripts on their own.
// =====================================================================================================================
extern "C" int mpvss_modp_group_has_device_share_hash(const mpvss_modp_group* grp) {
  if (rt_bad_group(grp)) return MPVSS_E_INVALID;
  return grp->has_sh ? 1 : 0;
}

extern "C" int mpvss_ctx_set_rt_share_hash(mpvss_ctx* ctx, int mode) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode < 0 || mode > 2) return fail(ctx, MPVSS_E_INVALID, "set_rt_share_hash: mode is 0, 1 or 2");
  ctx->rt_share_hash_mode = mode;
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_share_hash_stats(mpvss_ctx* ctx, unsigned long long* device_calls, unsigned long long* host_calls) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (device_calls) *device_calls = ctx->rt_share_hash_dev_calls;
  if (host_calls) *host_calls = ctx->rt_share_hash_host_calls;
  return MPVSS_OK;
}

// dleq.rs:87-126 for n transcripts: a caller's own DLEQ shape after group_dleq_commitments.  No host path inside.
extern "C" int mpvss_modp_group_dleq_challenges(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* h1,
                                                const uint8_t* h2, const uint8_t* a1, const uint8_t* a2, size_t n, uint8_t* c_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_dleq_challenges: no group");
  if (n == 0) return MPVSS_OK;
  if (!h1 || !h2 || !a1 || !a2 || !c_out || n > 0x7fffffff || (space != MPVSS_HOST && space != MPVSS_DEVICE))
    return fail(ctx, MPVSS_E_INVALID, "group_dleq_challenges: bad argument");
  if (!grp->has_sh) return fail(ctx, MPVSS_E_INVALID, RT_NO_SH);
  std::vector<uint8_t> c32;
  RtCall f(ctx, grp, space);
  RET_IF(f.begin(0));                                         // nothing here needs the constants of q
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* d1 = f.in(h1, off, cnt, ctx->rt_in[0], RtCall::Public);
    const uint8_t* d2 = f.in(h2, off, cnt, ctx->rt_in[1], RtCall::Public);
    const uint8_t* d3 = f.in(a1, off, cnt, ctx->rt_in[2], RtCall::Public);
    const uint8_t* d4 = f.in(a2, off, cnt, ctx->rt_in[3], RtCall::Public);
    if (!f.caller_on_host()) {                                // the caller's own array: EB bytes per share, written by the kernel
      RET_IF(f.rc);
      return rt_share_hash_dev(f, d1, d2, d3, d4, nullptr, cnt, nullptr, c_out + off * f.EB, f.EB);
    }
    uint8_t* dc32 = f.raw(ctx->rt_sh_c32, cnt * 32);
    RET_IF(f.rc);
    RET_IF(rt_share_hash_dev(f, d1, d2, d3, d4, nullptr, cnt, nullptr, dc32, 32));
    c32.resize(cnt * 32);
    f.host_bytes(c32.data(), dc32, cnt * 32);
    RET_IF(f.settle());
    rt_widen_challenges(c32.data(), cnt, f.EB, c_out + off * f.EB);
    return 0;
  }));
  return f.end();
}

// =====================================================================================================================
// Key sets of a run-time group (DESIGN section 13, "Key sets"): the rows of long-lived public keys, built once, and the calls
// that raise those keys to full-width powers over them -- a2_i = y_i^r_i Y_i^c of the verifier, Y_i = y_i^P(i) and a2_i = y_i^w_i
// of the dealer.  A set is explicit: the caller built it and names it, so nothing here decides by a threshold.
// =====================================================================================================================
extern "C" size_t mpvss_modp_group_keyset_bytes_per_key(const mpvss_modp_group* grp) {
  return rt_bad_group(grp) ? 0 : modp_rt_keyset_bytes(grp->lpl, 1);
}

extern "C" size_t mpvss_modp_group_keyset_bytes(const mpvss_modp_group_keyset* ks) {
  return ks ? modp_rt_keyset_bytes(ks->lpl, ks->n) : 0;
}

extern "C" int mpvss_modp_group_keyset_create(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* pubkeys, size_t n,
                                              mpvss_modp_group_keyset** out) {
  if (out) *out = nullptr;
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_keyset_create: no group");
  if (!out || !pubkeys || n == 0 || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_keyset_create: bad argument (n >= 1)");
  mpvss_modp_group_keyset* ks = new (std::nothrow) mpvss_modp_group_keyset();
  if (!ks) return fail(ctx, MPVSS_E_NOMEM, "group_keyset_create: no memory for the handle");
  ks->ctx = ctx;
  memcpy(ks->q_be, grp->q_be, sizeof(ks->q_be));
  ks->eb = grp->eb;
  ks->lpl = grp->lpl;
  ks->n = n;
  const int rc = [&]() -> int {
    RtCall f(ctx, grp, space);
    RET_IF(f.begin());
    const hipError_t e = hipMalloc((void**)&ks->rows, modp_rt_keyset_bytes(grp->lpl, n));
    if (e != hipSuccess) {
      (void)hipGetLastError();       // the runtime's last-error slot is sticky: the next launcher must not see this
      ks->rows = nullptr;
      return fail(ctx, MPVSS_E_NOMEM, "group_keyset_create: hipMalloc(rows)", e);
    }
    // a chunk's launch works on at most 2^20 keys, so that keys x rows fits the launcher's int
    const size_t step = std::min(MAX_CHUNK, (size_t)1 << 20), stride = rt_keyset_stride(grp);
    for (size_t off = 0; off < n; off += step) {
      const size_t cnt = std::min(n - off, step);
      const uint8_t* dk = f.in(pubkeys, off, cnt, ctx->rt_in[1], RtCall::Public);
      RET_IF(f.rc);
      TIMED_LAUNCH(ctx, 2, modp_rt_launch_keyset_build(grp->lpl, dk, (int)cnt, ks->rows + off * stride, f.dc, ctx->stream));
      RET_IF(f.settle());            // the staging buffer is reused by the next chunk
    }
    return f.end();
  }();
  if (rc != MPVSS_OK) {
    if (ks->rows) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipFree(ks->rows);
    }
    delete ks;
    return rc;
  }
  *out = ks;
  return MPVSS_OK;
}

// The run-time calls are synchronous: once the last call that named the set has returned, nothing reads its rows.
extern "C" void mpvss_modp_group_keyset_destroy(mpvss_ctx* ctx, mpvss_modp_group_keyset* ks) {
  if (!ks) return;
  mpvss_ctx* const owner = ks->ctx;          // the set is freed on its own context's device whichever context is named
  (void)ctx;
  std::lock_guard<std::mutex> lk(owner->mu);
  if (ks->rows && hipSetDevice(owner->device) == hipSuccess) {
    (void)hipStreamSynchronize(owner->stream);
    (void)hipFree(ks->rows);
  }
  delete ks;
}

extern "C" int mpvss_modp_group_keyset_dual_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space,
                                                const mpvss_modp_group_keyset* keyset, size_t key_offset, const uint8_t* e1,
                                                const uint8_t* h2, const uint8_t* e2, int e2_per_share, size_t n, uint8_t* out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_keyset_dual_exp: no group");
  const uint32_t* rows;
  RET_IF(rt_keyset_rows(ctx, grp, keyset, key_offset, n, &rows));
  if (n == 0) return MPVSS_OK;
  if (!e1 || !out || (h2 && !e2) || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_keyset_dual_exp: bad argument");
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  const uint8_t* dshared = nullptr;
  if (h2 && !e2_per_share) RET_IF(rt_stage_small(ctx, grp, e2, ctx->rt_small[1], &dshared));   // host bytes, as group_dleq_commitments' c
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* d1 = f.in(e1, off, cnt, ctx->rt_in[3], RtCall::Public);
    const uint8_t* dh = h2 ? f.in(h2, off, cnt, ctx->rt_in[2], RtCall::Public) : nullptr;
    const uint8_t* d2 = (h2 && e2_per_share) ? f.in(e2, off, cnt, ctx->rt_in[5], RtCall::Public) : dshared;
    uint8_t* dout = f.out(out, off, cnt, ctx->rt_out[0]);
    RET_IF(f.rc);
    const uint32_t* t2 = nullptr;
    if (h2) RET_IF(rt_tables(ctx, grp, f.dc, dh, f.EB, cnt, ctx->rt_tab2, &t2));
    TIMED_LAUNCH(ctx, 3, modp_rt_launch_keyset_exp(grp->lpl, rows + off * rt_keyset_stride(grp), t2, 16 * rt_L(grp), d1, nullptr, d2,
                                                   e2_per_share ? f.EB : 0, (int)cnt, dout, nullptr, f.dc, ctx->stream));
    return 0;
  }));
  return f.end();
}

extern "C" int mpvss_modp_group_keyset_twin_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space,
                                                const mpvss_modp_group_keyset* keyset, size_t key_offset, const uint8_t* e1,
                                                const uint8_t* e2, size_t n, uint8_t* out1, uint8_t* out2) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_keyset_twin_exp: no group");
  const uint32_t* rows;
  RET_IF(rt_keyset_rows(ctx, grp, keyset, key_offset, n, &rows));
  if (n == 0) return MPVSS_OK;
  if (!e1 || !e2 || !out1 || !out2 || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_keyset_twin_exp: bad argument");
  RtCall f(ctx, grp, space);
  RET_IF(f.begin());
  RET_IF(f.for_chunks(n, [&](size_t off, size_t cnt) {
    const uint8_t* d1 = f.in(e1, off, cnt, ctx->rt_in[2], RtCall::Secret);      // the dealer's P(i) and w_i, as group_batch_twin_exp's
    const uint8_t* d2 = f.in(e2, off, cnt, ctx->rt_in[3], RtCall::Secret);
    uint8_t* o1 = f.out(out1, off, cnt, ctx->rt_out[0]);
    uint8_t* o2 = f.out(out2, off, cnt, ctx->rt_out[1]);
    RET_IF(f.rc);
    TIMED_LAUNCH(ctx, 3, modp_rt_launch_keyset_exp(grp->lpl, rows + off * rt_keyset_stride(grp), nullptr, 0, d1, d2, nullptr, 0, (int)cnt,
                                                   o1, o2, f.dc, ctx->stream));
    return 0;
  }));
  return f.end();
}

extern "C" int mpvss_modp_group_verify_distribution_keyset(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space,
                                                           const uint8_t* commitments, size_t t, const int64_t* positions,
                                                           const mpvss_modp_group_keyset* keyset, size_t key_offset,
                                                           const uint8_t* shares, const uint8_t* responses, size_t n,
                                                           const uint8_t* challenge_host, int* verdict, uint8_t* digest32_out,
                                                           uint8_t* x_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_verify_distribution_keyset: no group");
  if (!verdict || !challenge_host || n > 0x7fffffff || t > 0x7fffffff ||
      (n > 0 && (!commitments || !positions || !shares || !responses || t == 0)))
    return fail(ctx, MPVSS_E_INVALID, "group_verify_distribution_keyset: bad argument");
  const uint32_t* rows;
  RET_IF(rt_keyset_rows(ctx, grp, keyset, key_offset, n, &rows));
  return rt_verify_distribution_locked(ctx, grp, space, commitments, t, positions, nullptr, rows, shares, responses, n, challenge_host,
                                       verdict, digest32_out, x_out_host, a1_out_host, a2_out_host);
}

extern "C" int mpvss_modp_group_deal_keyset(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t,
                                            const int64_t* positions_host, const mpvss_modp_group_keyset* keyset, size_t key_offset,
                                            const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out,
                                            uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out256, uint8_t* r_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_deal_keyset: no group");
  if (n > 0x7fffffff || t > 0x7fffffff || (n > 0 && (!coeffs_host || !positions_host || !witnesses_host || !y_out || !r_out || t == 0)))
    return fail(ctx, MPVSS_E_INVALID, "group_deal_keyset: bad argument (t >= 1, n < 2^31)");
  if (t > n) return fail(ctx, MPVSS_E_INVALID, "group_deal_keyset: threshold > number of public keys (participant.rs:166)");
  const uint32_t* rows;
  RET_IF(rt_keyset_rows(ctx, grp, keyset, key_offset, n, &rows));
  return rt_deal_locked(ctx, grp, coeffs_host, t, positions_host, nullptr, rows, witnesses_host, n, x_out, y_out, a1_out, a2_out,
                        digest32_out, challenge_out256, r_out);
}

// =====================================================================================================================
// Many boxes in one call (DESIGN section 13, "Many boxes in one call"): mpvss_modp_group_verify_many.  A PVSS round gives a
// verifier tens to hundreds of small boxes for the same keys; one box per call is the latency of a chain of Montgomery products
// on one or two waves.  Runs of small boxes therefore travel as ONE dense concatenation through the launches of one box:
// k_rt_to_mont over all commitments, k_rt_commit_eval_tiles (a tile = up to RT_NUMS shares of one box = one workgroup), the
// challenge of each box spread to its shares, then rt_dleq_dev with a per-share c.  Which boxes travel together: many::walk (host_many.h).
// =====================================================================================================================
namespace {

// The largest n and t of a box that may travel in a run: 16384, the group-14 figure.  The condition on it -- for no measured shape
// may the grouped call be slower than the loop of one-box calls -- holds with room at every shape of tools/modp_rt_many_boxes.py
// (profiles/modp_rt_many_boxes.txt: 400 x (5, 3) 159 .. 385 times faster, 200 x (100, 34) 18 .. 104 times, 60 x (1024, 32), the
// largest boxes measured, 5.6 .. 12.9 times, at 1024 and 2048 bits, host and device space, key arrays and one key set), so the
// value stays.  Boxes between 1024 and 16384 shares have not been measured.
constexpr size_t RT_GROUP_BOX_MAX = 16384;
constexpr size_t RT_TILE = 16;                     // RT_NUMS of modp_rt_kernels.inc: numbers per workgroup of every run-time kernel

enum RtBoxKind { RT_BOX_MALFORMED, RT_BOX_EMPTY, RT_BOX_SMALL, RT_BOX_SINGLE };

// one box, judged on the host before anything is launched
RtBoxKind rt_box_kind(const mpvss_ctx* ctx, const mpvss_modp_group* grp, const mpvss_modp_group_box& b) {
  if (!b.challenge_host || b.n > 0x7fffffff || b.t > 0x7fffffff) return RT_BOX_MALFORMED;
  if (b.n > 0 && (!b.commitments || !b.positions || !b.shares || !b.responses || b.t == 0 || (!b.keyset && !b.pubkeys)))
    return RT_BOX_MALFORMED;
  if (b.keyset && rt_keyset_refusal(ctx, grp, b.keyset, b.key_offset, b.n)) return RT_BOX_MALFORMED;
  if (b.n == 0) return RT_BOX_EMPTY;
  // a run holds at most MAX_CHUNK shares and as many commitments (its launchers count in int)
  return (b.n <= RT_GROUP_BOX_MAX && b.t <= RT_GROUP_BOX_MAX && b.n <= MAX_CHUNK && b.t <= MAX_CHUNK) ? RT_BOX_SMALL : RT_BOX_SINGLE;
}

// the one-box path, unchanged: chunking and forward differences included
int rt_many_single(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_box& b, int* verdict, uint8_t* digest) {
  const uint32_t* rows = nullptr;
  if (b.keyset) RET_IF(rt_keyset_rows(ctx, grp, b.keyset, b.key_offset, b.n, &rows));
  return rt_verify_distribution_locked(ctx, grp, space, b.commitments, b.t, b.positions, b.keyset ? nullptr : b.pubkeys, rows, b.shares,
                                       b.responses, b.n, b.challenge_host, verdict, digest, nullptr, nullptr, nullptr);
}

// one array of a run on the device, dense: gathered on the host and copied once (host space), or one device-to-device copy per
// box (device space).  piece(k, &src, &bytes): box k's part.
template <class Piece>
int rt_run_gather(mpvss_ctx* ctx, int space, size_t boxes, size_t total_bytes, DevBuf& buf, std::vector<uint8_t>& host, Piece piece) {
  RET_IF(ensure(ctx, buf, total_bytes));
  if (space == MPVSS_DEVICE) {
    size_t at = 0;
    for (size_t k = 0; k < boxes; ++k) {
      const void* src;
      size_t bytes;
      piece(k, &src, &bytes);
      HIPCHK(ctx, hipMemcpyAsync((uint8_t*)buf.p + at, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
      at += bytes;
    }
    return 0;
  }
  host.resize(total_bytes);
  size_t at = 0;
  for (size_t k = 0; k < boxes; ++k) {
    const void* src;
    size_t bytes;
    piece(k, &src, &bytes);
    memcpy(host.data() + at, src, bytes);
    at += bytes;
  }
  HIPCHK(ctx, hipMemcpyAsync(buf.p, host.data(), total_bytes, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

// a grouped pass: the boxes run[0 .. B) (indices into `boxes`, all RT_BOX_SMALL, all with array keys or all with the key set
// `ks`), shares in all <= MAX_CHUNK.  Same launches as one box, plus the spreading kernel.
int rt_many_run(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_box* boxes, const std::vector<size_t>& run,
                int hash_threads, int* verdicts, uint8_t* digests32) {
  const size_t B = run.size(), EB = grp->eb;
  const mpvss_modp_group_keyset* ks = boxes[run[0]].keyset;
  // the tables: tiles {box, first share, live count, 0}, boxes {first commitment, t}, and with a key set the key of every share
  std::vector<uint32_t> tiles, btab(2 * B), key_of;
  std::vector<size_t> first(B + 1), counts(B);
  size_t S = 0, T = 0;
  for (size_t k = 0; k < B; ++k) {
    const mpvss_modp_group_box& b = boxes[run[k]];
    first[k] = S;
    counts[k] = b.n;
    btab[2 * k] = (uint32_t)T;
    btab[2 * k + 1] = (uint32_t)b.t;
    if (ks)
      for (size_t i = 0; i < b.n; ++i) key_of.push_back((uint32_t)(b.key_offset + i));
    S += b.n;
    T += b.t;
  }
  first[B] = S;
  many::tile_table(counts.data(), B, RT_TILE, 4, tiles);
  const size_t ntiles = tiles.size() / 4;
  std::vector<uint8_t> ch(B * EB);
  for (size_t k = 0; k < B; ++k) memcpy(ch.data() + k * EB, boxes[run[k]].challenge_host, EB);

  // host sources of asynchronous copies and the results read back: declared before the frame, whose way out drains the stream
  std::vector<uint8_t> g_pos, g_cm, g_y, g_Y, g_r, hX, h1, h2, hYdev;
  std::vector<int64_t> pos_back;
  RtCall f(ctx, grp, space);
  StreamDrain drain{ctx};
  RET_IF(f.begin());
  auto part = [&](const uint8_t* mpvss_modp_group_box::*arr, size_t mpvss_modp_group_box::*cnt, size_t unit) {
    return [&run, boxes, arr, cnt, unit](size_t k, const void** src, size_t* bytes) {
      *src = boxes[run[k]].*arr;
      *bytes = boxes[run[k]].*cnt * unit;
    };
  };
  RET_IF(rt_run_gather(ctx, space, B, S * 8, ctx->rt_run_pos, g_pos, [&](size_t k, const void** src, size_t* bytes) {
    *src = boxes[run[k]].positions;
    *bytes = boxes[run[k]].n * 8;
  }));
  RET_IF(rt_run_gather(ctx, space, B, T * EB, ctx->rt_in[4], g_cm, part(&mpvss_modp_group_box::commitments, &mpvss_modp_group_box::t, EB)));
  if (!ks) RET_IF(rt_run_gather(ctx, space, B, S * EB, ctx->rt_in[1], g_y, part(&mpvss_modp_group_box::pubkeys, &mpvss_modp_group_box::n, EB)));
  RET_IF(rt_run_gather(ctx, space, B, S * EB, ctx->rt_in[2], g_Y, part(&mpvss_modp_group_box::shares, &mpvss_modp_group_box::n, EB)));
  RET_IF(rt_run_gather(ctx, space, B, S * EB, ctx->rt_in[3], g_r, part(&mpvss_modp_group_box::responses, &mpvss_modp_group_box::n, EB)));
  // positions are checked as the one-box call checks them: a negative one ends the call (the reference panics)
  const int64_t* P = (const int64_t*)g_pos.data();
  if (space == MPVSS_DEVICE) {
    pos_back.resize(S);
    HIPCHK(ctx, hipMemcpyAsync(pos_back.data(), ctx->rt_run_pos.p, S * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    P = pos_back.data();
  }
  RET_IF(check_positions_host(ctx, P, S));
  RET_IF(ensure(ctx, ctx->rt_run_tiles, tiles.size() * 4));
  RET_IF(ensure(ctx, ctx->rt_run_boxes, btab.size() * 4));
  RET_IF(ensure(ctx, ctx->rt_run_ch, B * EB));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_run_tiles.p, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_run_boxes.p, btab.data(), btab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_run_ch.p, ch.data(), B * EB, hipMemcpyHostToDevice, ctx->stream));
  if (ks) {
    RET_IF(ensure(ctx, ctx->rt_run_keyof, S * 4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rt_run_keyof.p, key_of.data(), S * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  uint8_t* dc_share = f.work(ctx->rt_in[5], S);
  uint8_t* dX = f.work(ctx->rt_out[0], S);
  uint8_t* d1 = f.work(ctx->rt_out[1], S);
  uint8_t* d2 = f.work(ctx->rt_out[2], S);
  RET_IF(f.rc);
  RET_IF(ensure(ctx, ctx->rt_cm, T * rt_L(grp) * 4));
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, (const uint8_t*)ctx->rt_in[4].p, (int)T, (uint32_t*)ctx->rt_cm.p, f.dc, ctx->stream));
  ++ctx->rt_horner_calls;
  TIMED_LAUNCH(ctx, 0, modp_rt_launch_commit_eval_tiles(grp->lpl, (const uint32_t*)ctx->rt_cm.p, (const uint32_t*)ctx->rt_run_tiles.p,
                                                        (int)ntiles, (const uint32_t*)ctx->rt_run_boxes.p,
                                                        (const int64_t*)ctx->rt_run_pos.p, dX, f.dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_spread_challenge((const uint8_t*)ctx->rt_run_ch.p, (const uint32_t*)ctx->rt_run_tiles.p, (int)ntiles, (int)EB,
                                                 dc_share, ctx->stream));
  // a1 = g^r X^c, a2 = y^r Y^c over the concatenation, every share with its own box's c
  RET_IF(rt_dleq_dev(ctx, grp, f.dc, grp->g_be, dX, ks ? nullptr : (const uint8_t*)ctx->rt_in[1].p, ks ? ks->rows : nullptr,
                     (const uint8_t*)ctx->rt_in[2].p, (const uint8_t*)ctx->rt_in[3].p, dc_share, EB, S, d1, d2,
                     ks ? (const uint32_t*)ctx->rt_run_keyof.p : nullptr));
  f.to_host(dX, S, hX);
  f.to_host(d1, S, h1);
  f.to_host(d2, S, h2);
  const uint8_t* Y = g_Y.data();
  if (space == MPVSS_DEVICE) {
    f.to_host((const uint8_t*)ctx->rt_in[2].p, S, hYdev);
    Y = hYdev.data();
  }
  RET_IF(f.settle());
  // the boxes' transcripts are independent: box k hashes the shares first[k] .. first[k+1] of the concatenation
  // automatic: one thread per 512 shares of the run (half a megabyte of transcript and more), never sized by the machine
  const size_t nth = std::min<size_t>((size_t)many::many_threads(hash_threads, S, 512), B);
  hsc::parallel_indices((unsigned)nth, [&](unsigned slice) {
    for (size_t k = B * slice / nth; k < B * (slice + 1) / nth; ++k) {
      mpvss::Sha256 h;
      frame_shares(h, hX.data(), Y, h1.data(), h2.data(), first[k], first[k + 1], EB);
      uint8_t digest[32], c[RT_EB_MAX];
      h.final(digest);
      if (digests32) memcpy(digests32 + 32 * run[k], digest, 32);
      rt_hash_to_scalar(grp, digest, 32, c);
      verdicts[run[k]] = memcmp(c, boxes[run[k]].challenge_host, EB) == 0 ? 1 : 0;
    }
  });
  ++ctx->rt_many_groups;
  ctx->rt_many_grouped_boxes += B;
  return f.end();
}

}  // namespace

extern "C" int mpvss_modp_group_verify_many(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_box* boxes,
                                            size_t count, int hash_threads, int* verdicts, uint8_t* digests32) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_verify_many: no group");
  if (count == 0) return MPVSS_OK;
  if (!boxes || !verdicts) return fail(ctx, MPVSS_E_INVALID, "group_verify_many: bad argument");
  for (size_t i = 0; i < count; ++i) verdicts[i] = 0;
  if (digests32) memset(digests32, 0, 32 * count);         // a malformed box has no transcript: verdict 0, digest zero
  // The runs of many::walk: small boxes that take keys the same way (arrays, or one and the same key set) travel together, (n, t)
  // against MAX_CHUNK shares and MAX_CHUNK commitments.  Malformed boxes are settled above and empty ones on the host (the empty
  // transcript); neither ends a run.  A run of one box takes the one-box path, like every box that fits no run.
  return many::walk(
      count, MAX_CHUNK, MAX_CHUNK,
      [&](size_t i) {
        const RtBoxKind kind = rt_box_kind(ctx, grp, boxes[i]);
        return kind == RT_BOX_MALFORMED ? many::SKIP : kind == RT_BOX_EMPTY ? many::ASIDE : kind == RT_BOX_SINGLE ? many::ALONE : many::GROUPED;
      },
      [&](size_t i) { return many::Cost{boxes[i].n, boxes[i].t}; },
      [&](size_t first, size_t i) { return boxes[first].keyset == boxes[i].keyset; },
      [&](size_t i) -> int {
        RET_IF(rt_many_single(ctx, grp, space, boxes[i], &verdicts[i], digests32 ? digests32 + 32 * i : nullptr));
        if (boxes[i].n > 0) ++ctx->rt_many_single_boxes;        // (an empty box ran nothing)
        return MPVSS_OK;
      },
      [&](const std::vector<size_t>& run) { return rt_many_run(ctx, grp, space, boxes, run, hash_threads, verdicts, digests32); });
}

extern "C" int mpvss_modp_group_verify_many_stats(mpvss_ctx* ctx, unsigned long long* groups, unsigned long long* grouped_boxes,
                                                  unsigned long long* single_boxes) {
  return many_stats(ctx, &mpvss_ctx::rt_many_groups, &mpvss_ctx::rt_many_grouped_boxes, &mpvss_ctx::rt_many_single_boxes, groups,
                    grouped_boxes, single_boxes);
}

// =====================================================================================================================
// Many secrets in one call (DESIGN section 13, "Many secrets in one call"): mpvss_modp_group_reconstruct_many.  After verifying, a
// participant of a PVSS round reconstructs one secret per dealer, usually from the same responding participants: one secret per
// call is the latency of a chain of Montgomery products plus ceil(log2 m) rounds of the pairwise product, on one or two waves,
// and the same m Lagrange coefficients computed again by every call.  Here the coefficients are computed once per distinct
// position list, and runs of secrets travel as ONE dense concatenation of shares through the launches of one secret, the
// pairwise rounds replaced by one k_rt_product_segments launch (one workgroup per secret).  The plan of the position lists and the
// walk that forms the passes: many::plan_secrets, many::walk_secrets (host_many.h).
// =====================================================================================================================
namespace {

// a grouped pass: the secrets run[0 .. B) (indices into `secrets`, all many::SECRET_GROUPED), shares in all <= MAX_CHUNK.  The
// launches of one secret over the concatenation, then one k_rt_product_segments launch and one settle.  A secret with a share that
// is 0 mod q under a negative coefficient is refused here (the one copy back of a pass in device space shows it): its powers run
// with the others, its result is dropped.
int rt_reconstruct_pass(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_secret* secrets,
                        const std::vector<size_t>& run, const std::vector<many::SecretPlan>& plan, const uint8_t* exps,
                        const uint8_t* exps_dev, const char* negs, int host_threads, int* status, uint8_t* gs_out, uint8_t* masks_out32) {
  const size_t B = run.size(), EB = grp->eb;
  std::vector<uint32_t> segs(2 * B);                                // {first factor, m} of every secret
  std::vector<size_t> first(B + 1);
  size_t S = 0;
  for (size_t k = 0; k < B; ++k) {
    first[k] = S;
    segs[2 * k] = (uint32_t)S;
    segs[2 * k + 1] = (uint32_t)secrets[run[k]].m;
    S += secrets[run[k]].m;
  }
  first[B] = S;
  // host sources of asynchronous copies and the results read back: declared before the frame, whose way out drains the stream
  std::vector<uint8_t> g_sh, g_exp(exps_dev ? 0 : S * EB), h_sh, h_gs;
  if (!exps_dev)
    for (size_t k = 0; k < B; ++k) memcpy(g_exp.data() + first[k] * EB, exps + plan[run[k]].coef * EB, secrets[run[k]].m * EB);
  RtCall f(ctx, grp, space);
  StreamDrain drain{ctx};
  RET_IF(f.begin());
  RET_IF(rt_run_gather(ctx, space, B, S * EB, ctx->rt_in[0], g_sh, [&](size_t k, const void** src, size_t* bytes) {
    *src = secrets[run[k]].shares;
    *bytes = secrets[run[k]].m * EB;
  }));
  const uint8_t* dS = (const uint8_t*)ctx->rt_in[0].p;
  // a share that is 0 mod q has no inverse: the reference returns None when its coefficient is negative (:551-553)
  const uint8_t* Sv = g_sh.data();
  if (space == MPVSS_DEVICE) {
    f.to_host(dS, S, h_sh);
    RET_IF(f.host_ready());
    Sv = h_sh.data();
  }
  std::vector<char> refused(B, 0);
  size_t good = 0;
  for (size_t k = 0; k < B; ++k) {
    const char* neg = negs + plan[run[k]].coef;
    for (size_t i = 0; i < secrets[run[k]].m && !refused[k]; ++i)
      if (neg[i] && rt_zero_mod_q(grp, Sv + (first[k] + i) * EB)) refused[k] = 1;
    if (!refused[k]) ++good;
  }
  // the exponents: the host's, or gathered device to device from the call's coefficient buffer, one copy per secret
  const uint8_t* dE = exps_dev ? f.work(ctx->rt_in[1], S) : f.in_host(g_exp.data(), S, ctx->rt_in[1], RtCall::Public);
  uint8_t* dF = f.work(ctx->rt_out[0], S);
  uint8_t* dG = f.work(ctx->rt_out[1], B);
  RET_IF(f.rc);
  if (exps_dev)
    for (size_t k = 0; k < B; ++k)
      HIPCHK(ctx, hipMemcpyAsync((uint8_t*)ctx->rt_in[1].p + first[k] * EB, exps_dev + plan[run[k]].coef * EB, secrets[run[k]].m * EB,
                                 hipMemcpyDeviceToDevice, ctx->stream));
  RET_IF(ensure(ctx, ctx->rt_run_boxes, segs.size() * 4));
  HIPCHK(ctx, hipMemcpyAsync(ctx->rt_run_boxes.p, segs.data(), segs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  RET_IF(ensure(ctx, ctx->rt_tab1, S * rt_L(grp) * 4));
  const uint32_t* tb;
  RET_IF(rt_tables(ctx, grp, f.dc, dS, EB, S, ctx->rt_tab2, &tb));
  RET_IF(rt_dual_exp_any(ctx, grp, 3, tb, 16 * rt_L(grp), nullptr, 0, dE, EB, nullptr, 0, S, dF, f.dc));   // S_i^lambda_i, every secret
  LAUNCHCHK(ctx, modp_rt_launch_to_mont(grp->lpl, dF, (int)S, (uint32_t*)ctx->rt_tab1.p, f.dc, ctx->stream));
  LAUNCHCHK(ctx, modp_rt_launch_product_segments(grp->lpl, (const uint32_t*)ctx->rt_tab1.p, (const uint32_t*)ctx->rt_run_boxes.p, (int)B,
                                                 dG, f.dc, ctx->stream));                              // one product per secret
  f.to_host(dG, B, h_gs);
  RET_IF(f.settle());
  hsc::parallel_for(B, many::many_threads(host_threads, B, 256), [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      if (refused[k]) continue;
      const size_t i = run[k];
      memcpy(gs_out + i * EB, h_gs.data() + k * EB, EB);
      if (masks_out32) rt_secret_mask(grp, h_gs.data() + k * EB, masks_out32 + 32 * i);
      status[i] = MPVSS_OK;
    }
  });
  for (size_t k = 0; k < B; ++k)
    if (refused[k]) status[run[k]] = MPVSS_E_INVALID;
  if (good) {
    ++ctx->rt_rec_passes;
    ctx->rt_rec_grouped_secrets += good;
  }
  return f.end();
}

}  // namespace

extern "C" int mpvss_modp_group_reconstruct_many(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space,
                                                 const mpvss_modp_group_secret* secrets, size_t count, int host_threads, int* status,
                                                 uint8_t* gs_out, uint8_t* masks_out32) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_reconstruct_many: no group");
  if (count == 0) return MPVSS_OK;
  if (!secrets || !status || !gs_out) return fail(ctx, MPVSS_E_INVALID, "group_reconstruct_many: bad argument");
  const size_t EB = grp->eb;
  // a refused secret has no result: its status, zeros in gs and in its mask.  Every secret is refused until it has its result.
  for (size_t i = 0; i < count; ++i) status[i] = MPVSS_E_INVALID;
  memset(gs_out, 0, count * EB);
  if (masks_out32) memset(masks_out32, 0, 32 * count);

  // the Lagrange exponents and their signs ONCE per distinct position list (a list without them has duplicate positions, or a
  // denominator without inverse -- an even (q-1)/2 among the causes: its secrets are refused): on the host threads of the call, or
  // by ONE pass of launches over all lists into a buffer of the context that the passes gather from
  many::SecretPlans lists = many::plan_lists(secrets, count, RT_GROUP_BOX_MAX, MAX_CHUNK);
  double work = 0;
  for (const size_t lm : lists.list_m) work += (double)lm * (double)lm;
  const bool on_device = !lists.list_m.empty() &&
                         rt_lagrange_on_device(ctx, grp, work, *std::max_element(lists.list_m.begin(), lists.list_m.end()), lists.coefs);
  std::vector<uint8_t> exps;
  std::vector<char> negs;
  const uint8_t* exps_dev = nullptr;
  ctx->call_spans.spans.clear();
  ctx->call_spans.ev_used = 0;
  if (on_device) {
    negs.assign(lists.coefs, 0);
    std::vector<char> list_ok(lists.list_m.size(), 0);
    hsc::parallel_for(list_ok.size(), many::many_threads(host_threads, lists.coefs, 4096), [&](size_t lo, size_t hi) {
      for (size_t l = lo; l < hi; ++l)
        list_ok[l] = rt_lagrange_signs(lists.list_pos[l], lists.list_m[l], negs.data() + lists.list_first[l]) ? 1 : 0;
    });
    std::vector<int64_t> all_pos(lists.coefs);               // coefficient c belongs to position c; a refused list has no tile
    std::vector<RtLagrangeList> admitted;
    std::vector<size_t> admitted_l;
    for (size_t l = 0; l < list_ok.size(); ++l) {
      memcpy(all_pos.data() + lists.list_first[l], lists.list_pos[l], lists.list_m[l] * 8);
      if (!list_ok[l]) continue;
      admitted.push_back(RtLagrangeList{lists.list_first[l], lists.list_m[l], lists.list_pos[l]});
      admitted_l.push_back(l);
    }
    if (!admitted.empty()) {
      struct SpanGuard {                                     // the launches' spans outlive the passes, which reset the main ones
        mpvss_ctx* c;
        ~SpanGuard() { c->sp = &c->main_spans; }
      } guard{ctx};
      ctx->sp = &ctx->call_spans;
      RtCall f(ctx, grp, space);
      RET_IF(f.begin(RtCall::SubQ));
      RET_IF(ensure(ctx, ctx->rt_lag_call_exp, lists.coefs * EB));
      std::vector<char> ok(admitted.size(), 1);
      RET_IF(rt_lagrange_dev(f, ctx->rt_lag_call_pos, ctx->rt_lag_call_tiles, ctx->rt_lag_call_neg, all_pos.data(), negs.data(), lists.coefs,
                             admitted, (uint8_t*)ctx->rt_lag_call_exp.p, ok));
      for (size_t k = 0; k < ok.size(); ++k) list_ok[admitted_l[k]] = ok[k];
    }
    many::plan_settle(lists, list_ok);
    exps_dev = (const uint8_t*)ctx->rt_lag_call_exp.p;
  } else {
    many::plan_host_coefficients(lists, host_threads,
                                 [&](size_t coefs) {
                                   exps.resize(coefs * EB);
                                   negs.assign(coefs, 0);
                                 },
                                 [&](const int64_t* pos, size_t m, size_t j, size_t c) { return rt_lagrange_exponent(grp, pos, m, j, exps.data() + c * EB, &negs[c]); });
    std::vector<char> counted(lists.list_m.size(), 0);
    for (size_t i = 0; i < count; ++i)
      if (lists.secret[i].kind == many::SECRET_GROUPED && !counted[lists.list_of[i]]) {
        counted[lists.list_of[i]] = 1;
        ++ctx->rt_lagrange_host_lists;
      }
  }
  const std::vector<many::SecretPlan>& plan = lists.secret;
  // A code of the one-secret path other than MPVSS_E_INVALID (which refuses that secret alone) ends the call.
  auto single = [&](size_t i) -> int {
    const mpvss_modp_group_secret& s = secrets[i];
    const bool pre = plan[i].coef != (size_t)-1;             // a run of one: its list's exponents are there already
    const int rc = rt_reconstruct_locked(ctx, grp, space, s.positions_host, s.shares, s.m, gs_out + i * EB,
                                         masks_out32 ? masks_out32 + 32 * i : nullptr,
                                         pre && !exps_dev ? exps.data() + plan[i].coef * EB : nullptr, pre ? negs.data() + plan[i].coef : nullptr,
                                         pre && exps_dev ? exps_dev + plan[i].coef * EB : nullptr);
    if (rc == MPVSS_E_INVALID) return MPVSS_OK;
    RET_IF(rc);
    status[i] = MPVSS_OK;
    ++ctx->rt_rec_single_secrets;
    return MPVSS_OK;
  };
  RET_IF(many::walk_secrets(secrets, plan, MAX_CHUNK, single, [&](const std::vector<size_t>& run) {
    return rt_reconstruct_pass(ctx, grp, space, secrets, run, plan, exps.data(), exps_dev, negs.data(), host_threads, status, gs_out, masks_out32);
  }));
  if (!ctx->call_spans.spans.empty()) {                       // the coefficient launches among the kernel times of the call's last pass
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    double sum = 0;
    for (auto& sp : ctx->call_spans.spans) {
      float ms = 0;
      HIPCHK(ctx, hipEventElapsedTime(&ms, sp.a, sp.b));
      sum += ms;
    }
    ctx->kernel_ms[4] = (ctx->kernel_ms[4] > 0 ? ctx->kernel_ms[4] : 0) + sum;
    ctx->kernel_launches[4] += (int)ctx->call_spans.spans.size();
  }
  return MPVSS_OK;
}

// ---- where the Lagrange exponents of a run-time group are computed, and the device path on its own ------------------------------
extern "C" int mpvss_ctx_set_rt_lagrange(mpvss_ctx* ctx, int mode) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode < 0 || mode > 2) return fail(ctx, MPVSS_E_INVALID, "set_rt_lagrange: mode is 0, 1 or 2");
  const int before = ctx->rt_lagrange_mode;
  ctx->rt_lagrange_mode = mode;
  return before;
}

extern "C" int mpvss_modp_group_lagrange_stats(mpvss_ctx* ctx, unsigned long long* device_lists, unsigned long long* host_lists,
                                               unsigned long long* fallback_lists) {
  return many_stats(ctx, &mpvss_ctx::rt_lagrange_dev_lists, &mpvss_ctx::rt_lagrange_host_lists, &mpvss_ctx::rt_lagrange_fallback_lists,
                    device_lists, host_lists, fallback_lists);
}

extern "C" int mpvss_modp_group_lagrange_exponents(mpvss_ctx* ctx, const mpvss_modp_group* grp, const int64_t* positions_host, size_t m,
                                                   uint8_t* exps_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (rt_bad_group(grp)) return fail(ctx, MPVSS_E_INVALID, "group_lagrange_exponents: no group");
  if (!positions_host || !exps_out_host || m == 0 || m > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "group_reconstruct: bad argument");
  for (size_t i = 0; i < m; ++i)
    if (positions_host[i] < 1) return fail(ctx, MPVSS_E_INVALID, "group_reconstruct: positions must be >= 1 (util.rs:47-64)");
  std::vector<char> neg;
  std::vector<uint8_t> exps;                                 // the output stays untouched by a refused call
  RtCall f(ctx, grp, MPVSS_HOST);
  RET_IF(f.begin(0));
  const uint8_t* exps_dev = nullptr;
  RET_IF(rt_lagrange_one(f, positions_host, m, exps, neg, &exps_dev));
  if (exps_dev) {
    f.to_host(exps_dev, m, exps);
    RET_IF(f.settle());
  }
  RET_IF(f.end());
  memcpy(exps_out_host, exps.data(), m * grp->eb);
  return MPVSS_OK;
}

// ---- the row layout for small calls: mode, the automatic bound of a handle, launches through the wrappers ----------------------------
extern "C" int mpvss_ctx_set_rt_row(mpvss_ctx* ctx, int mode) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode < 0 || mode > 2) return fail(ctx, MPVSS_E_INVALID, "set_rt_row: mode is 0, 1 or 2");
  const int before = ctx->rt_row_mode;
  ctx->rt_row_mode = mode;
  return before;
}

extern "C" int mpvss_modp_group_row_max_shares(const mpvss_modp_group* grp) { return rt_bad_group(grp) ? 0 : (int)rt_row_max_shares(grp->lpl); }

extern "C" int mpvss_modp_group_row_stats(mpvss_ctx* ctx, unsigned long long* row_launches, unsigned long long* quad_launches) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (row_launches) *row_launches = ctx->rt_row_launches;
  if (quad_launches) *quad_launches = ctx->rt_quad_launches;
  return MPVSS_OK;
}

extern "C" int mpvss_modp_group_reconstruct_many_stats(mpvss_ctx* ctx, unsigned long long* passes, unsigned long long* grouped_secrets,
                                                       unsigned long long* single_secrets) {
  return many_stats(ctx, &mpvss_ctx::rt_rec_passes, &mpvss_ctx::rt_rec_grouped_secrets, &mpvss_ctx::rt_rec_single_secrets, passes,
                    grouped_secrets, single_secrets);
}
