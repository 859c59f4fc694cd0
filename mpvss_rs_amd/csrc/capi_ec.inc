// =====================================================================================================
// Elliptic-curve groups: secp256k1 (src/groups/secp256k1.rs) and ristretto255 (src/groups/ristretto255.rs)
// Part of mpvss_capi.cpp (included at its end): same context, workspaces, block slots and pipeline.
// =====================================================================================================
#include <limits.h>

#include "ec_kernels.h"
#include "sha512.h"

// A key set of a curve group (include/mpvss_hip.h, "Key sets of a curve group"): the per-key combs of n public keys on the
// device (ec_launch_keyset_build) and a mark per key that is the identity.  It belongs to the context that built it, remembers
// its curve and never changes after create.  The rows hold public values only and are not wiped.
struct mpvss_ec_keyset {
  mpvss_ctx* ctx = nullptr;
  int group = 0;
  size_t n = 0;
  uint32_t* rows = nullptr;      // [n][65][8][packed affine words]
  uint8_t* marks = nullptr;      // [n]: 1 = the key is the identity
};

namespace {

struct EcInfo {
  int group;
  size_t enc;            // element bytes
  bool scalar_be;        // scalar byte order
  uint8_t order_be[32];  // group order, big-endian
  uint8_t gen[33];       // canonical encoding of the generator
};

const EcInfo* ec_info(int group) {
  static const EcInfo secp = {
      MPVSS_GROUP_SECP256K1, 33, true,
      {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFE,
       0xBA, 0xAE, 0xDC, 0xE6, 0xAF, 0x48, 0xA0, 0x3B, 0xBF, 0xD2, 0x5E, 0x8C, 0xD0, 0x36, 0x41, 0x41},   // secp256k1.rs:47-51
      {0x02, 0x79, 0xBE, 0x66, 0x7E, 0xF9, 0xDC, 0xBB, 0xAC, 0x55, 0xA0, 0x62, 0x95, 0xCE, 0x87, 0x0B, 0x07,
       0x02, 0x9B, 0xFC, 0xDB, 0x2D, 0xCE, 0x28, 0xD9, 0x59, 0xF2, 0x81, 0x5B, 0x16, 0xF8, 0x17, 0x98}};
  static const EcInfo rist = {
      MPVSS_GROUP_RISTRETTO255, 32, false,
      {0x10, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00,
       0x14, 0xde, 0xf9, 0xde, 0xa2, 0xf7, 0x9c, 0xd6, 0x58, 0x12, 0x63, 0x1a, 0x5c, 0xf5, 0xd3, 0xed},   // ristretto255.rs:55-59
      {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f, 0x58,
       0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76, 0x00}};
  if (group == MPVSS_GROUP_SECP256K1) return &secp;
  if (group == MPVSS_GROUP_RISTRETTO255) return &rist;
  return nullptr;
}

// scalar (in the group's byte order) < group order ?
bool scalar_canonical(const EcInfo* gi, const uint8_t* s) {
  for (int i = 0; i < 32; ++i) {
    const uint8_t a = gi->scalar_be ? s[i] : s[31 - i];
    if (a != gi->order_be[i]) return a < gi->order_be[i];
  }
  return false;
}

// Group::hash_to_scalar(data) in the group's scalar byte order:
//   secp256k1     SHA-256 -> big-endian integer -> mod n (secp256k1.rs:121-131); 2^256 < 2n, one subtraction suffices
//   ristretto255  SHA-512 -> 64-byte little-endian integer -> mod l (ristretto255.rs:196-205): bitwise long division
void ec_hash_to_scalar_bytes(const EcInfo* gi, const uint8_t* data, size_t len, uint8_t out[32]) {
  if (gi->group == MPVSS_GROUP_SECP256K1) {
    uint8_t h[32];
    mpvss::sha256(data, len, h);
    if (!scalar_canonical(gi, h)) {
      int borrow = 0;
      for (int i = 31; i >= 0; --i) {
        const int d = (int)h[i] - gi->order_be[i] - borrow;
        h[i] = (uint8_t)(d & 0xff);
        borrow = d < 0;
      }
    }
    memcpy(out, h, 32);
    return;
  }
  uint8_t wide[64];
  mpvss::sha512(data, len, wide);
  uint64_t l[4] = {0, 0, 0, 0};
  for (int i = 0; i < 32; ++i) l[3 - i / 8] |= (uint64_t)gi->order_be[i] << (8 * (7 - i % 8));
  uint64_t r[5] = {0, 0, 0, 0, 0};
  for (int bit = 511; bit >= 0; --bit) {
    for (int k = 4; k > 0; --k) r[k] = (r[k] << 1) | (r[k - 1] >> 63);
    r[0] = (r[0] << 1) | ((wide[bit >> 3] >> (bit & 7)) & 1);
    bool ge = r[4] != 0;
    if (!ge) {
      ge = true;
      for (int k = 3; k >= 0; --k)
        if (r[k] != l[k]) { ge = r[k] > l[k]; break; }
    }
    if (ge) {
      unsigned __int128 borrow = 0;
      for (int k = 0; k < 4; ++k) {
        const unsigned __int128 d = (unsigned __int128)r[k] - l[k] - (uint64_t)borrow;
        r[k] = (uint64_t)d;
        borrow = (d >> 64) & 1;
      }
      r[4] -= (uint64_t)borrow;
    }
  }
  for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(r[i / 8] >> (8 * (i % 8)));
}

// the reference's callers pass the 32-byte transcript digest as `data` (participant.rs:1436, 1879)
void ec_hash_to_scalar(const EcInfo* gi, const uint8_t digest[32], uint8_t out[32]) {
  ec_hash_to_scalar_bytes(gi, digest, 32, out);
}

inline void ec_frame_update(mpvss::Sha256& h, const uint8_t* e, size_t len) {
  uint8_t pre[8] = {0, 0, 0, 0, 0, 0, 0, (uint8_t)len};      // dleq.rs:58-61: u64 big-endian length
  h.update(pre, 8);
  h.update(e, len);
}

// framed(X_i) | framed(Y_i) | framed(a1_i) | framed(a2_i) for shares [i0, i1), L-byte encodings: a run of shares' frames side by side
// in a cache-resident buffer, one update per run (eight 8- and 33-byte updates per share otherwise: 20 % more time per box)
inline void ec_frame_shares(mpvss::Sha256& h, const uint8_t* X, const uint8_t* Y, const uint8_t* a1, const uint8_t* a2, size_t L, size_t i0,
                            size_t i1) {
  constexpr size_t RUN = 128;
  uint8_t buf[RUN * 4 * (33 + 8)];
  for (size_t i = i0; i < i1; i += RUN) {
    const size_t e = i + RUN < i1 ? i + RUN : i1;
    uint8_t* w = buf;
    for (size_t k = i; k < e; ++k)
      for (const uint8_t* a : {X, Y, a1, a2}) {
        memset(w, 0, 7);
        w[7] = (uint8_t)L;                                   // dleq.rs:58-61: u64 big-endian length
        memcpy(w + 8, a + k * L, L);
        w += 8 + L;
      }
    h.update(buf, (size_t)(w - buf));
  }
}

EcWork& ecw(mpvss_ctx* ctx) { return ctx->ecwork; }

int ec_report_bad_element(mpvss_ctx* ctx, const char* what, size_t i) {
  char buf[200];
  snprintf(buf, sizeof(buf), "%s: element %zu is not a valid group-element encoding", what, i);
  return fail(ctx, MPVSS_E_INVALID, buf);
}
int ec_report_bad_scalar(mpvss_ctx* ctx, const char* what, size_t i) {
  char buf[200];
  snprintf(buf, sizeof(buf), "%s: scalar %zu is not below the group order (the reference cannot represent it)", what, i);
  return fail(ctx, MPVSS_E_INVALID, buf);
}

int ec_check_ok(mpvss_ctx* ctx, const uint8_t* ok_dev, size_t n, const char* what) {
  std::vector<uint8_t> h(n);
  HIPCHK(ctx, hipMemcpyAsync(h.data(), ok_dev, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; ++i)
    if (!h[i]) return ec_report_bad_element(ctx, what, i);
  return 0;
}

int ec_check_scalars(mpvss_ctx* ctx, const EcInfo* gi, int space, const uint8_t* s, size_t n, const char* what) {
  std::vector<uint8_t> h;
  RET_IF(small_vec_to_host(ctx, space, s, n * 32, h));
  for (size_t i = 0; i < n; ++i)
    if (!scalar_canonical(gi, h.data() + i * 32)) return ec_report_bad_scalar(ctx, what, i);
  return 0;
}

// commitments (encoded, `space`) -> decoded points in w.cm; ok flags to ok_dev (checked by the caller)
int ec_stage_commitments_async(mpvss_ctx* ctx, const EcInfo* gi, EcWork& w, int space, const uint8_t* commitments, size_t t,
                               uint8_t* ok_dev) {
  const void* dc;
  RET_IF(stage_in(ctx, space, commitments, t * gi->enc, w.cmenc, &dc));
  RET_IF(ensure(ctx, w.cm, t * (size_t)ec_point_words(gi->group) * 4));
  LAUNCHCHK(ctx, ec_launch_decode(gi->group, (const uint8_t*)dc, (int)t, (uint32_t*)w.cm.p, ok_dev, ctx->stream));
  return 0;
}
int ec_stage_commitments(mpvss_ctx* ctx, const EcInfo* gi, EcWork& w, int space, const uint8_t* commitments, size_t t) {
  RET_IF(ensure(ctx, w.ok, t > 4096 ? t : 4096));
  RET_IF(ec_stage_commitments_async(ctx, gi, w, space, commitments, t, (uint8_t*)w.ok.p));
  return ec_check_ok(ctx, (const uint8_t*)w.ok.p, t, "commitments");
}

int ec_generator_dev(mpvss_ctx* ctx, const EcInfo* gi, EcWork& w, const uint8_t* gen_host, const uint8_t** dev) {
  RET_IF(ensure(ctx, w.gen, 64));
  HIPCHK(ctx, hipMemcpyAsync(w.gen.p, gen_host ? gen_host : gi->gen, gi->enc, hipMemcpyHostToDevice, ctx->stream));
  *dev = (const uint8_t*)w.gen.p;
  return 0;
}

// fixed-base comb of the group's generator (65 windows x 8 packed affine entries), built once per context
int ec_comb(mpvss_ctx* ctx, int group, const uint32_t** comb) {
  const int gx = group - 1;
  if (!ctx->ec_comb_ready[gx]) {
    RET_IF(ensure(ctx, ctx->ec_comb[gx], (size_t)ec_comb_words(group) * 4));
    LAUNCHCHK(ctx, ec_launch_comb_build(group, (uint32_t*)ctx->ec_comb[gx].p, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // once per context: every stream reads the table afterwards
    ctx->ec_comb_ready[gx] = true;
  }
  *comb = (const uint32_t*)ctx->ec_comb[gx].p;
  return 0;
}

// One base of a double-scalar multiplication: the group generator (comb), encoded points (enc_stride 0 = one shared
// point) and / or points in internal coordinates (both given: `gate` tells the kernels which is valid).
struct EcBase {
  bool generator = false;
  const uint32_t* table = nullptr;     // a window table built by an earlier call for the same bases: used as is
  const uint8_t* enc = nullptr;
  size_t enc_stride = 0;
  const uint32_t* pts = nullptr;
  const int* gate = nullptr;
};

// out_enc[x] = k1[x] * B1[x] + k2[x] * B2[x] for n shares on ctx->stream (b2 == null: out = k1 * B1).
// Window tables go to tabA / tabB, the internal results to pout; ok1 / ok2 (device, n bytes each, may be null) receive
// the validity of decoded bases.  out_enc may be null: the results stay in pout alone.
int ec_dual(mpvss_ctx* ctx, const EcInfo* gi, const EcBase& b1, const uint8_t* k1, size_t k1_stride, const EcBase* b2,
            const uint8_t* k2, size_t k2_stride, size_t n, DevBuf& tabA, DevBuf& tabB, DevBuf& pout, uint8_t* out_enc,
            uint8_t* ok1, uint8_t* ok2) {
  const int group = gi->group;
  const size_t tab_bytes = n * 8 * (size_t)ec_cached_words(group) * 4;
  const uint32_t *comb = nullptr, *t1 = nullptr, *t2 = nullptr;
  if (b1.generator) {
    RET_IF(ec_comb(ctx, group, &comb));
    if (ok1 != nullptr) HIPCHK(ctx, hipMemsetAsync(ok1, 1, n, ctx->stream));
  } else if (b1.table != nullptr) {
    t1 = b1.table;
    if (ok1 != nullptr) HIPCHK(ctx, hipMemsetAsync(ok1, 1, n, ctx->stream));
  } else {
    RET_IF(ensure(ctx, tabA, tab_bytes));
    if (b1.enc == nullptr && ok1 != nullptr) HIPCHK(ctx, hipMemsetAsync(ok1, 1, n, ctx->stream));
    TIMED_LAUNCH(ctx, 2, ec_launch_build_tables(group, b1.enc, b1.enc_stride, b1.pts, (int)n, (uint32_t*)tabA.p, ok1, b1.gate,
                                                ctx->stream));
    t1 = (const uint32_t*)tabA.p;
  }
  if (b2 != nullptr) {
    RET_IF(ensure(ctx, tabB, tab_bytes));
    if (b2->enc == nullptr && ok2 != nullptr) HIPCHK(ctx, hipMemsetAsync(ok2, 1, n, ctx->stream));
    TIMED_LAUNCH(ctx, 2, ec_launch_build_tables(group, b2->enc, b2->enc_stride, b2->pts, (int)n, (uint32_t*)tabB.p, ok2,
                                                b2->gate, ctx->stream));
    t2 = (const uint32_t*)tabB.p;
  } else if (ok2 != nullptr) {
    HIPCHK(ctx, hipMemsetAsync(ok2, 1, n, ctx->stream));
  }
  RET_IF(ensure(ctx, pout, n * (size_t)ec_point_words(group) * 4));
  TIMED_LAUNCH(ctx, 1, ec_launch_dual_win(group, comb, t1, k1, k1_stride, t2, k2, k2_stride, (int)n, (uint32_t*)pout.p,
                                          ctx->stream));
  // (out_enc == null: the caller goes on with the internal points in pout and nobody reads the encodings -- a reconstruct pass)
  if (out_enc != nullptr) TIMED_LAUNCH(ctx, 3, ec_launch_encode(group, (const uint32_t*)pout.p, (int)n, out_enc, ctx->stream));
  return 0;
}

// One byte per key beside its rows: the identity mark.
constexpr size_t EC_KEYSET_MARK_BYTES = 1;

// The one admission of a key set to a call (context lock held): built by this context, for this curve, and holding the keys
// key_offset .. key_offset + n - 1.  Why not, or null when the set is admitted.
const char* ec_keyset_refusal(const mpvss_ctx* ctx, int group, const mpvss_ec_keyset* ks, size_t key_offset, size_t n) {
  if (!ks) return "key set: none given";
  if (ks->ctx != ctx) return "key set: built by another context";
  if (ks->group != group) return "key set: built for the other curve";
  if (key_offset > ks->n || n > ks->n - key_offset) return "key set: key_offset + n is beyond the set";
  return nullptr;
}

// out1[x] = k1[x] * y_(first + x) and (k2 != null) out2[x] = k2[x] * y_(first + x), x < n, in internal coordinates on
// ctx->stream: one walk over the rows, both scalar sets in one launch.  The counter feeds mpvss_ec_keyset_stats.
int ec_keyset_walk(mpvss_ctx* ctx, const mpvss_ec_keyset* ks, size_t first, const uint8_t* k1, const uint8_t* k2, size_t n,
                   uint32_t* out1, uint32_t* out2) {
  TIMED_LAUNCH(ctx, 1, ec_launch_keyset_walk(ks->group, ks->rows + first * ec_keyset_row_words(ks->group), ks->marks + first, k1, k2,
                                             (int)n, out1, out2, ctx->stream));
  ctx->ec_ks_powers += (k2 != nullptr ? 2 : 1) * (unsigned long long)n;
  return 0;
}

// may the forward differences serve a curve box of this shape?  MPVSS_EC_FD=0 disables the path.
bool ec_fd_shape(size_t n, size_t t) {
  static const int fd_on = fd_env("MPVSS_EC_FD", 1);
  return fd_on && t >= 16 && t <= 256 && n >= 16 * t && n >= 4096;
}

// S strided chains of chain_len members cover a box's n positions; each chain's t seeds start at member w0 and it steps both ways
struct EcFdGeometry {
  int S, chain_len, w0;
  size_t state_words;       // difference tables of a box: forward and backward per chain, and those of the two-level seeding
};
EcFdGeometry ec_fd_geometry(int group, size_t n, size_t t) {
  EcFdGeometry g;
  g.S = std::max((int)(4096 / t), 4);
  const int s_max = (int)(n / (4 * t));
  if (g.S > s_max) g.S = s_max;
  if (g.S < 1) g.S = 1;
  g.chain_len = (int)((n + g.S - 1) / g.S);
  g.w0 = (g.chain_len - (int)t) / 2;
  g.state_words = ((size_t)2 * g.S * t + 2 * t) * (size_t)ec_point_words(group);
  return g;
}

// What the forward-difference X path of B boxes of one shape works on: box b at b * its stride of every array (sized by the caller
// from ec_fd_geometry; no stride matters when B = 1).  hand / wtab: the optional buffers of the quad-lane pipelines, sized here.
struct EcFdBoxes {
  const uint32_t* cm;       // decoded commitments
  const int64_t* pos;
  uint32_t* pts;            // out: internal points
  uint32_t* state;
  uint8_t* xenc;            // out: encodings
  int* flags;               // the boxes' gates
  const int* ones;          // B ones in PINNED memory: the gates are initialised by an asynchronous copy
  DevBuf &hand, &wtab;
  size_t cm_stride, pos_stride, pts_stride, state_stride, enc_stride;
};

// X of B boxes of one shape (n, t; ec_fd_shape holds) by forward differences on stream s, ONE sequence of launches with the box as
// the second grid dimension.
//   device_positions : nobody has looked at the positions: a kernel checks each box's and clears its gate unless they are consecutive
//   may_quad         : the caller's part of the MPVSS_EC_FD_QUAD = 1 condition (the chip is the boxes' own)
//   two_level        : the caller's reading of MPVSS_EC_FD_L1
//   timed            : the launches are spans of ctx's timing (s must be ctx->stream then), else plain launches
// *gate_out = the gates (box b: + b) when the boxes have them -- then Horner's rule has filled in for every box whose gate
// was cleared -- or null: the forward differences ran unconditionally.
#define EC_X_LAUNCH(call)                           \
  do {                                              \
    if (timed) TIMED_LAUNCH(ctx, 0, call);          \
    else LAUNCHCHK(ctx, call);                      \
  } while (0)
int ec_fd_x(mpvss_ctx* ctx, const EcInfo* gi, const EcFdBoxes& bx, size_t B, size_t n, size_t t, const EcFdGeometry& g,
            bool device_positions, bool may_quad, bool two_level, hipStream_t s, bool timed, const int** gate_out) {
  constexpr int split_seeds = 1;     // every seed evaluated by 8 lanes (shorter latency)
  const int group = gi->group;
  const size_t pw = (size_t)ec_point_words(group);
  // Boxes that have the chip to themselves step through pipelines of quad-lane stages (ec_quad.h): a third of the latency per step.
  // MPVSS_EC_FD_QUAD: 0 never, 1 when the caller allows it, 2 always; the pipeline may give up, so it always has a gate.
  static const int quad_mode = fd_env("MPVSS_EC_FD_QUAD", 1), quad_fault = fd_env("MPVSS_EC_FD_TEST_FAULT", 0);
  constexpr int quad_seeds = 1;     // its seed kernel: 16 lanes per seed, windowed x^lo
  constexpr int quad_table = 1;     // its difference tables by the same pipeline
  constexpr int quad_oct = 0;       // (secp256k1 with eight lanes per point was built, exact and 4 % slower: profiles/r04_ec_quad_isa.txt)
  const bool quad = quad_mode >= 2 || (quad_mode == 1 && may_quad);
  const int* gate = nullptr;
  if (device_positions || quad) {       // every box decides for itself on the device / a flag the stepping pipeline can clear
    HIPCHK(ctx, hipMemcpyAsync(bx.flags, bx.ones, B * 4, hipMemcpyHostToDevice, s));
    if (device_positions)
      for (size_t b = 0; b < B; ++b)
        LAUNCHCHK(ctx, modp_launch_fd_check_positions(bx.pos + b * bx.pos_stride, (int)n, bx.flags + b, s));
    gate = bx.flags;
  }
  EcQuadStepping qs{nullptr, 0, bx.flags, quad_fault};
  bool use_quad = quad;       // (its hand-over space is a few hundred MB: without it the one-workgroup-per-chain kernels run)
  if (use_quad) {
    qs.oct = quad_oct;
    qs.hand_box_words = ec_fd_quad_hand_words(group, quad_oct, (int)t, g.S, g.w0, g.chain_len);
    // (a chain of n / S members keeps every handed point: 160 B x 15 x 2 S x its steps -- 177 MB at n = 65536, 2.8 GB at 2^20; beyond
    // 4 GB the chain kernels run)
    if (B * qs.hand_box_words * 4 > ((size_t)4 << 30) || !try_ensure(ctx, bx.hand, B * qs.hand_box_words * 4)) use_quad = false;
    qs.hand = (uint32_t*)bx.hand.p;
    if (use_quad && quad_seeds) {
      qs.wtab_box_words = ec_fd_seed_tab_words(group, two_level ? (int)t : g.S * (int)t);
      if (try_ensure(ctx, bx.wtab, B * qs.wtab_box_words * 4)) qs.wtab = (uint32_t*)bx.wtab.p;
    }
    qs.table = quad_table;
  }
  uint32_t* st = bx.state;
  EC_X_LAUNCH(ec_launch_fd_boxes_q(group, bx.cm, (int)t, bx.pos, (int)n, g.S, g.w0, g.chain_len, bx.pts, st, st + (size_t)g.S * t * pw,
                                   two_level ? st + (size_t)2 * g.S * t * pw : nullptr, bx.xenc, split_seeds, gate, (int)B, bx.cm_stride,
                                   bx.pos_stride, bx.pts_stride, bx.state_stride, bx.enc_stride, use_quad ? &qs : nullptr, s));
  if (gate != nullptr)         // fallback per box: Horner's rule when its positions are not consecutive (or its pipeline gave up)
    EC_X_LAUNCH(ec_launch_commit_eval_boxes(group, bx.cm, (int)t, bx.pos, (int)n, bx.xenc, gate, 0, (int)B, bx.cm_stride, bx.pos_stride,
                                            bx.enc_stride, s));
  *gate_out = gate;
  return 0;
}
#undef EC_X_LAUNCH

// X_i for n shares: encodings into dX and, when the forward-difference path runs, internal points in w.pts.
//   hpos != null : positions known to the host, the choice is made here           -> *gate_out = null unless the quad pipeline runs
//   hpos == null : positions are device-resident; a kernel checks them and a device flag (w.flags[0]) gates the two
//                  paths (no host synchronisation)                                 -> *gate_out = the flag
// *pts_out = w.pts when the internal points may be valid (always valid if *gate_out == null), else null.
int ec_eval_x(mpvss_ctx* ctx, const EcInfo* gi, EcWork& w, size_t t, const int64_t* hpos, const int64_t* dpos, size_t n,
              uint8_t* dX, const int** gate_out, const uint32_t** pts_out) {
  const int group = gi->group;
  *gate_out = nullptr;
  *pts_out = nullptr;
  if (!ec_fd_shape(n, t) || (hpos != nullptr && !positions_consecutive(hpos, n))) {
    TIMED_LAUNCH(ctx, 0, ec_launch_commit_eval(group, (const uint32_t*)w.cm.p, (int)t, dpos, (int)n, dX, nullptr, 0, ctx->stream));
    return 0;
  }
  const EcFdGeometry g = ec_fd_geometry(group, n, t);
  RET_IF(ensure(ctx, w.flags, 64));
  RET_IF(ensure(ctx, w.pts, n * (size_t)ec_point_words(group) * 4));
  RET_IF(ensure(ctx, w.fdst, g.state_words * 4));
  // Two-level seeding (Horner for t seeds only, the others by a stride-1 chain) removes 37 % of a box's instructions but
  // adds a serial chain to its latency (X path 24 -> 39 ms for a lone secp256k1 box): worth it when other blocks keep the
  // chip busy, not for a call that has the GPU to itself.  MPVSS_EC_FD_L1: 0 never, 1 when blocks are in flight, 2 always.
  static const int l1_mode = fd_env("MPVSS_EC_FD_L1", 1);
  const bool two_level = l1_mode >= 2 || (l1_mode == 1 && ctx->busy_with_others());
  ctx->w->root[0].one = 1;     // pinned constant of the current workspace: the gate's copy is asynchronous
  const EcFdBoxes bx{(const uint32_t*)w.cm.p, dpos, (uint32_t*)w.pts.p, (uint32_t*)w.fdst.p, dX, (int*)w.flags.p, &ctx->w->root[0].one,
                     w.hand, w.wtab, 0, 0, 0, 0, 0};
  // (the quad pipelines: a call that has the chip to itself, no other block in flight)
  RET_IF(ec_fd_x(ctx, gi, bx, 1, n, t, g, hpos == nullptr, !ctx->busy_with_others(), two_level, ctx->stream, true, gate_out));
  *pts_out = (const uint32_t*)w.pts.p;
  return 0;
}

}  // namespace

#define EC_PROLOGUE(what)                                                             \
  if (!ctx) return MPVSS_E_INVALID;                                                   \
  std::lock_guard<std::mutex> lk(ctx->mu);                                            \
  const EcInfo* gi = ec_info(group);                                                  \
  if (!gi) return fail(ctx, MPVSS_E_UNSUPPORTED, what ": unknown group");             \
  HIPCHK(ctx, hipSetDevice(ctx->device));                                             \
  EcWork& w = ecw(ctx);                                                               \
  spans_reset(ctx)

// ---- Group::exp / Group::mul -----------------------------------------------------------------------
extern "C" int mpvss_ec_batch_exp(mpvss_ctx* ctx, int group, int space, const uint8_t* bases, const uint8_t* scalars,
                                  size_t n, uint8_t* out) {
  EC_PROLOGUE("ec_batch_exp");
  if (n == 0) return MPVSS_OK;
  if (!bases || !scalars || !out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_batch_exp: bad argument");
  RET_IF(ec_check_scalars(ctx, gi, space, scalars, n, "ec_batch_exp"));
  const void *db, *dk;
  RET_IF(stage_in(ctx, space, bases, n * gi->enc, w.a, &db));
  RET_IF(stage_in(ctx, space, scalars, n * 32, w.b, &dk));
  uint8_t* dout = out;
  if (space == MPVSS_HOST) { RET_IF(ensure(ctx, w.o1, n * gi->enc)); dout = (uint8_t*)w.o1.p; }
  RET_IF(ensure(ctx, w.ok, n > 4096 ? n : 4096));
  EcBase b1;
  b1.enc = (const uint8_t*)db;
  b1.enc_stride = gi->enc;
  RET_IF(ec_dual(ctx, gi, b1, (const uint8_t*)dk, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p1, dout, (uint8_t*)w.ok.p, nullptr));
  if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, out, dout, n * gi->enc));
  RET_IF(ec_check_ok(ctx, (const uint8_t*)w.ok.p, n, "ec_batch_exp bases"));
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

// out[i] = scalars[i] * G: the shape of keygen (secp256k1.rs:168-171, ristretto255.rs:239-242), commitments
// C_j = a_j G (participant.rs:1145-1152) and a1 = w G -- fixed-base comb, no doublings
extern "C" int mpvss_ec_batch_exp_generator(mpvss_ctx* ctx, int group, int space, const uint8_t* scalars, size_t n,
                                            uint8_t* out) {
  EC_PROLOGUE("ec_batch_exp_generator");
  if (n == 0) return MPVSS_OK;
  if (!scalars || !out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_batch_exp_generator: bad argument");
  RET_IF(ec_check_scalars(ctx, gi, space, scalars, n, "ec_batch_exp_generator"));
  const void* dk;
  RET_IF(stage_in(ctx, space, scalars, n * 32, w.b, &dk));
  uint8_t* dout = out;
  if (space == MPVSS_HOST) { RET_IF(ensure(ctx, w.o1, n * gi->enc)); dout = (uint8_t*)w.o1.p; }
  EcBase g;
  g.generator = true;
  RET_IF(ec_dual(ctx, gi, g, (const uint8_t*)dk, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p1, dout, nullptr, nullptr));
  if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, out, dout, n * gi->enc));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

extern "C" int mpvss_ec_batch_mul(mpvss_ctx* ctx, int group, int space, const uint8_t* a, const uint8_t* b, size_t n,
                                  uint8_t* out) {
  EC_PROLOGUE("ec_batch_mul");
  if (n == 0) return MPVSS_OK;
  if (!a || !b || !out || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_batch_mul: bad argument");
  const void *da, *db;
  RET_IF(stage_in(ctx, space, a, n * gi->enc, w.a, &da));
  RET_IF(stage_in(ctx, space, b, n * gi->enc, w.b, &db));
  uint8_t* dout = out;
  if (space == MPVSS_HOST) { RET_IF(ensure(ctx, w.o1, n * gi->enc)); dout = (uint8_t*)w.o1.p; }
  RET_IF(ensure(ctx, w.ok, n > 4096 ? n : 4096));
  LAUNCHCHK(ctx, ec_launch_add(group, (const uint8_t*)da, (const uint8_t*)db, (int)n, dout, (uint8_t*)w.ok.p, ctx->stream));
  if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, out, dout, n * gi->enc));
  RET_IF(ec_check_ok(ctx, (const uint8_t*)w.ok.p, n, "ec_batch_mul operands"));
  return MPVSS_OK;
}

namespace {
// positions for the synchronous entry points: device copy + (host callers) the host view for the path decision.
// The curve groups turn a position into a scalar with `Scalar::from(position as u64)` (participant.rs:1182, 1419,
// 1862): a negative i64 wraps to a large u64 and the call goes on, unlike MODP where it panics -- so no sign check.
int ec_stage_positions(mpvss_ctx* ctx, EcWork& w, int space, const int64_t* positions, size_t n, const int64_t** dpos,
                       const int64_t** hpos) {
  const void* d;
  RET_IF(stage_in(ctx, space, positions, n * 8, w.pos, &d));
  *dpos = (const int64_t*)d;
  *hpos = space == MPVSS_HOST ? positions : nullptr;
  return 0;
}
}  // namespace

// ---- X_i = sum_j i^j C_j ------------------------------------------------------------------------------
extern "C" int mpvss_ec_commit_eval(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                    const int64_t* positions, size_t n, uint8_t* x_out) {
  EC_PROLOGUE("ec_commit_eval");
  if (n == 0) return MPVSS_OK;
  if (!commitments || !positions || !x_out || t == 0 || t > 0x7fffffff || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "ec_commit_eval: bad argument (t must be >= 1)");
  RET_IF(ec_stage_commitments(ctx, gi, w, space, commitments, t));
  const int64_t *dpos, *hpos;
  RET_IF(ec_stage_positions(ctx, w, space, positions, n, &dpos, &hpos));
  uint8_t* dout = x_out;
  if (space == MPVSS_HOST) { RET_IF(ensure(ctx, w.x, n * gi->enc)); dout = (uint8_t*)w.x.p; }
  const int* gate;
  const uint32_t* pts;
  RET_IF(ec_eval_x(ctx, gi, w, t, hpos, dpos, n, dout, &gate, &pts));
  if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, x_out, dout, n * gi->enc));
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

// ---- DLEQ verifier commitments --------------------------------------------------------------------------
extern "C" int mpvss_ec_dleq_commitments(mpvss_ctx* ctx, int group, int space, const uint8_t* g1_host, const uint8_t* h1,
                                         const uint8_t* g2, const uint8_t* h2, const uint8_t* r, const uint8_t* c,
                                         int c_per_share, size_t n, uint8_t* a1_out, uint8_t* a2_out) {
  EC_PROLOGUE("ec_dleq_commitments");
  if (n == 0) return MPVSS_OK;
  if (!g1_host || !h1 || !g2 || !h2 || !r || !c || !a1_out || !a2_out || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "ec_dleq_commitments: bad argument");
  RET_IF(ec_check_scalars(ctx, gi, space, r, n, "responses"));
  RET_IF(ec_check_scalars(ctx, gi, c_per_share ? space : MPVSS_HOST, c, c_per_share ? n : 1, "challenge"));
  const uint8_t* dg;
  RET_IF(ec_generator_dev(ctx, gi, w, g1_host, &dg));
  const void *dh1, *dg2, *dh2, *dr, *dc;
  RET_IF(stage_in(ctx, space, h1, n * gi->enc, w.a, &dh1));
  RET_IF(stage_in(ctx, space, g2, n * gi->enc, w.b, &dg2));
  RET_IF(stage_in(ctx, space, h2, n * gi->enc, w.c, &dh2));
  RET_IF(stage_in(ctx, space, r, n * 32, w.d, &dr));
  if (c_per_share) RET_IF(stage_in(ctx, space, c, n * 32, w.e, &dc)); else RET_IF(stage_in(ctx, MPVSS_HOST, c, 32, w.chal, &dc));
  uint8_t *d1 = a1_out, *d2 = a2_out;
  if (space == MPVSS_HOST) {
    RET_IF(ensure(ctx, w.o1, n * gi->enc)); RET_IF(ensure(ctx, w.o2, n * gi->enc));
    d1 = (uint8_t*)w.o1.p; d2 = (uint8_t*)w.o2.p;
  }
  const size_t okn = n > 4096 ? n : 4096;
  RET_IF(ensure(ctx, w.ok, 4 * okn));
  uint8_t* ok = (uint8_t*)w.ok.p;
  const size_t cs = c_per_share ? 32 : 0;
  EcBase bg, bh1, bg2, bh2;
  bg.generator = memcmp(g1_host, gi->gen, gi->enc) == 0;      // the group generator: fixed-base comb
  bg.enc = dg;
  bg.enc_stride = 0;
  bh1.enc = (const uint8_t*)dh1; bh1.enc_stride = gi->enc;
  bg2.enc = (const uint8_t*)dg2; bg2.enc_stride = gi->enc;
  bh2.enc = (const uint8_t*)dh2; bh2.enc_stride = gi->enc;
  RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dr, 32, &bh1, (const uint8_t*)dc, cs, n, w.tab1, w.tab2, w.p1, d1, ok, ok + n));
  RET_IF(ec_dual(ctx, gi, bg2, (const uint8_t*)dr, 32, &bh2, (const uint8_t*)dc, cs, n, w.tab1, w.tab2, w.p2, d2, ok + 2 * n,
                 ok + 3 * n));
  if (space == MPVSS_HOST) {
    RET_IF(copy_out(ctx, space, a1_out, d1, n * gi->enc));
    RET_IF(copy_out(ctx, space, a2_out, d2, n * gi->enc));
  }
  RET_IF(ec_check_ok(ctx, ok, 4 * n, "ec_dleq_commitments elements"));
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

// ---- verify_distribution_shares (participant.rs:1384-1442 secp256k1, 1827-1885 ristretto255) --------------
// Split like the MODP path: compute (enqueue only: X path on the slot's high-priority stream, a2 beside it on the
// low-priority one, a1 after X), absorb (wait, validity flags, ordered SHA-256), verdict.
namespace {

struct EcStaging {          // layout of a kind-2 slot's pinned staging
  uint8_t *X, *Y, *a1, *a2;
  int* flags;               // [0] gate (-1: no device decision), [1] first bad response, [2] first bad challenge
  uint8_t* ok;              // t (commitments) + n (public keys) + n (shares)
  uint8_t* in;              // host callers: copies of the inputs
  size_t out_bytes;
};
size_t ec_staging_out_bytes(size_t n, size_t t, size_t L) {
  return ((4 * n * L + 15) / 16) * 16 + 16 + ((t + 2 * n + 15) / 16) * 16;
}
EcStaging ec_staging(void* pin, size_t n, size_t t, size_t L) {
  EcStaging s;
  s.X = (uint8_t*)pin;
  s.Y = s.X + n * L;
  s.a1 = s.Y + n * L;
  s.a2 = s.a1 + n * L;
  size_t off = ((4 * n * L + 15) / 16) * 16;
  s.flags = (int*)((uint8_t*)pin + off);
  off += 16;
  s.ok = (uint8_t*)pin + off;
  off += ((t + 2 * n + 15) / 16) * 16;
  s.in = (uint8_t*)pin + off;
  s.out_bytes = off;
  return s;
}

// X of one box as a batch launch left it (ec_x_batch_compute): encodings, internal points, the box's gate and the
// validity flags of its commitments, all in the batch's workspace; `ready` fires when they are there
struct EcPre {
  const uint8_t* x_enc;
  const uint32_t* x_pts;
  const int* gate;
  const uint8_t* ok_cm;
  hipEvent_t ready;
};

// may this box's X path join a batch of boxes of shape (n, t)?  (forward differences must apply: the conditions of
// ec_eval_x; host positions are judged here, device positions by the box's gate on the device)
bool ec_x_box_batchable(int space, const mpvss_ec_box& bx, size_t n, size_t t) {
  if (bx.n != n || bx.t != t || !ec_fd_shape(n, t) || n > 0x7fffffff) return false;
  if (!bx.commitments || !bx.positions) return false;
  return space != MPVSS_HOST || positions_consecutive(bx.positions, n);
}

// The X paths of B boxes of one shape (same n, t; forward differences apply) by ONE sequence of launches with the box
// as the second grid dimension: a box's X path is a chain of narrow launches -- 32 workgroups stepping for 15 ms --
// and the device runs only eight launches side by side, so B boxes per launch is B times the work in flight
// (profiles/r02_ec_streams_ab.txt).  Returns MPVSS_OK with pre[0..B) filled, or 1 when the batch form does not apply
// (the caller then takes the per-box path).
int ec_x_batch_compute(mpvss_ctx* ctx, const EcInfo* gi, int space, const mpvss_ec_box* bx, size_t B, mpvss_ctx::XBatch& xb,
                       EcPre* pre) {
  static const bool two_level = fd_env("MPVSS_EC_FD_L1", 1) != 0;     // (any setting but 0: a batch does not ask what else is in flight)
  // quad-lane stepping pipelines (ec_fd_x) for a batch of one or two boxes with nothing else in flight
  const bool may_quad = B <= 2 && !ctx->busy_with_others();
  const size_t n = bx[0].n, t = bx[0].t, L = gi->enc;
  for (size_t b = 0; b < B; ++b)
    if (!ec_x_box_batchable(space, bx[b], n, t)) return 1;
  const int group = gi->group;
  const size_t pw = (size_t)ec_point_words(group);
  const EcFdGeometry g = ec_fd_geometry(group, n, t);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!xb.s) {
    HIPCHK(ctx, hipStreamCreateWithPriority(&xb.s, hipStreamNonBlocking, ctx->prio_high));
    HIPCHK(ctx, hipEventCreateWithFlags(&xb.done, hipEventDisableTiming));
  }
  RET_IF(ensure(ctx, xb.cmenc, B * t * L));
  RET_IF(ensure(ctx, xb.cm, B * t * pw * 4));
  RET_IF(ensure(ctx, xb.okcm, B * t));
  RET_IF(ensure(ctx, xb.pos, B * n * 8));
  RET_IF(ensure(ctx, xb.pts, B * n * pw * 4));
  RET_IF(ensure(ctx, xb.xenc, B * n * L));
  RET_IF(ensure(ctx, xb.state, B * g.state_words * 4));
  RET_IF(ensure(ctx, xb.flags, (B + 16) * 4));
  const size_t pin_need = (B + 16) * 4 + (space == MPVSS_HOST ? B * (t * L + n * 8) : 0);
  if (pin_need > xb.pin_cap) {
    if (xb.pin) HIPCHK(ctx, hipHostFree(xb.pin));
    xb.pin = nullptr;
    xb.pin_cap = 0;
    hipError_t e = hipHostMalloc(&xb.pin, pin_need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx, MPVSS_E_NOMEM, "hipHostMalloc(batch staging)", e);
    xb.pin_cap = pin_need;
  }
  hipStream_t s = xb.s;
  int* hones = (int*)xb.pin;
  for (size_t b = 0; b < B; ++b) hones[b] = 1;
  uint8_t* hin = (uint8_t*)xb.pin + (B + 16) * 4;
  for (size_t b = 0; b < B; ++b) {
    uint8_t* dcm = (uint8_t*)xb.cmenc.p + b * t * L;
    int64_t* dpos = (int64_t*)xb.pos.p + b * n;
    if (space == MPVSS_HOST) {
      memcpy(hin, bx[b].commitments, t * L);
      HIPCHK(ctx, hipMemcpyAsync(dcm, hin, t * L, hipMemcpyHostToDevice, s));
      hin += t * L;
      memcpy(hin, bx[b].positions, n * 8);
      HIPCHK(ctx, hipMemcpyAsync(dpos, hin, n * 8, hipMemcpyHostToDevice, s));
      hin += n * 8;
    } else {
      HIPCHK(ctx, hipMemcpyAsync(dcm, bx[b].commitments, t * L, hipMemcpyDeviceToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dpos, bx[b].positions, n * 8, hipMemcpyDeviceToDevice, s));
    }
  }
  LAUNCHCHK(ctx, ec_launch_decode(group, (const uint8_t*)xb.cmenc.p, (int)(B * t), (uint32_t*)xb.cm.p, (uint8_t*)xb.okcm.p, s));
  const EcFdBoxes fb{(const uint32_t*)xb.cm.p, (const int64_t*)xb.pos.p, (uint32_t*)xb.pts.p, (uint32_t*)xb.state.p, (uint8_t*)xb.xenc.p,
                     (int*)xb.flags.p, hones, xb.hand, xb.wtab, t * pw, n, n * pw, g.state_words, n * L};
  const int* gate;
  // (plain launches: the timing spans belong to the context's stream, not to this one)
  RET_IF(ec_fd_x(ctx, gi, fb, B, n, t, g, space != MPVSS_HOST, may_quad, two_level, s, false, &gate));
  HIPCHK(ctx, hipEventRecord(xb.done, s));
  for (size_t b = 0; b < B; ++b)
    pre[b] = EcPre{(const uint8_t*)xb.xenc.p + b * n * L, (const uint32_t*)xb.pts.p + b * n * pw, gate ? gate + b : nullptr,
                   (const uint8_t*)xb.okcm.p + b * t, xb.done};
  return MPVSS_OK;
}

int ec_verify_block_compute_locked(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                   const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                   const uint8_t* responses, size_t n, const uint8_t* challenge_host,
                                   const EcPre* pre = nullptr) {
  const EcInfo* gi = ec_info(group);
  if (!gi) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_verify: unknown group");
  if (!challenge_host) return fail(ctx, MPVSS_E_INVALID, "ec_verify: null challenge");
  if (n > 0 && (!commitments || !positions || !pubkeys || !shares || !responses || t == 0 || t > 0x7fffffff || n > 0x7fffffff))
    return fail(ctx, MPVSS_E_INVALID, "ec_verify_distribution: bad argument (t must be >= 1)");
  BlockEnqueue be(ctx, 2, n, "ec_verify");
  RET_IF(be.rc);
  mpvss_ctx::BlockSlot& sl = be.sl;
  sl.group = group;
  sl.t = t;
  if (n == 0) return be.commit_empty();
  if (!scalar_canonical(gi, challenge_host)) return ec_report_bad_scalar(ctx, "challenge", 0);
  const uint32_t* comb;
  RET_IF(ec_comb(ctx, group, &comb));          // before the streams are switched: built once on the context's stream
  RET_IF(be.enter());
  EcWork& w = sl.ecw;
  const size_t L = gi->enc;
  RET_IF(be.pin(ec_staging_out_bytes(n, t, L) + (space == MPVSS_HOST ? 2 * n * L + n * 32 + t * L + n * 8 : 0)));
  EcStaging st = ec_staging(sl.pin, n, t, L);
  const int64_t* hpos = nullptr;
  if (space == MPVSS_HOST) {       // pinned copies: every transfer is asynchronous, nothing of the caller's is kept
    uint8_t* in = st.in;
    memcpy(in, pubkeys, n * L); pubkeys = in; in += n * L;
    memcpy(in, shares, n * L); shares = in; in += n * L;
    memcpy(in, responses, n * 32); responses = in; in += n * 32;
    memcpy(in, commitments, t * L); commitments = in; in += t * L;
    memcpy(in, positions, n * 8); positions = (const int64_t*)in;
    hpos = positions;
  }
  const size_t okn = t + 2 * n;
  RET_IF(ensure(ctx, w.ok, okn));
  RET_IF(ensure(ctx, w.flags, 64));
  uint8_t* ok = (uint8_t*)w.ok.p;
  int* flags = (int*)w.flags.p;
  st.flags[0] = -1;
  st.flags[1] = st.flags[2] = INT_MAX;
  HIPCHK(ctx, hipMemcpyAsync(flags + 1, st.flags + 1, 8, hipMemcpyHostToDevice, ctx->stream));
  if (!pre) RET_IF(ec_stage_commitments_async(ctx, gi, w, space, commitments, t, ok));
  const void *dpos_v, *dy, *dY, *dr;
  RET_IF(stage_in(ctx, space, positions, n * 8, w.pos, &dpos_v));
  RET_IF(stage_in(ctx, space, pubkeys, n * L, w.a, &dy));
  RET_IF(stage_in(ctx, space, shares, n * L, w.b, &dY));
  RET_IF(stage_in(ctx, space, responses, n * 32, w.d, &dr));
  RET_IF(ensure(ctx, w.chal, 64));
  memcpy(sl.work.root[0].challenge, challenge_host, 32);
  HIPCHK(ctx, hipMemcpyAsync(w.chal.p, sl.work.root[0].challenge, 32, hipMemcpyHostToDevice, ctx->stream));
  const uint8_t* dc = (const uint8_t*)w.chal.p;
  LAUNCHCHK(ctx, verdict_launch_check_scalars(group, (const uint8_t*)dr, (int)n, flags + 1, ctx->stream));
  RET_IF(ensure(ctx, w.x, n * L));
  RET_IF(ensure(ctx, w.o1, n * L));
  RET_IF(ensure(ctx, w.o2, n * L));
  // no reallocation once two streams are live
  const size_t tab_bytes = n * 8 * (size_t)ec_cached_words(group) * 4, pts_bytes = n * (size_t)ec_point_words(group) * 4;
  RET_IF(ensure(ctx, w.tab1, tab_bytes));
  RET_IF(ensure(ctx, w.tab2, tab_bytes));
  RET_IF(ensure(ctx, w.tab3, tab_bytes));
  RET_IF(ensure(ctx, w.p1, pts_bytes));
  RET_IF(ensure(ctx, w.p2, pts_bytes));
  RET_IF(ensure(ctx, w.pg, pts_bytes));      // the generator half of a split a1: sized here, not under the fork (ensure() may free and synchronise)
  uint8_t *dX = (uint8_t*)w.x.p, *d1 = (uint8_t*)w.o1.p, *d2 = (uint8_t*)w.o2.p;
  // a2 = r*y + c*Y does not depend on X: it runs beside the X path on the slot's low-priority stream   (dleq.rs:79-81)
  // (keeping a block to one stream once several are in flight was measured slower: 5.2 against 6.3 M share verifications/s for
  // secp256k1, profiles/r02_ec_streams_ab.txt)
  // a block that has the chip to itself: the generator half of a1 = r G + c X runs beside the X path
  const bool split_a1 = !ctx->busy_with_others();
  hipStream_t side = sl.work.sb;
  RET_IF(fork_side_stream(ctx, sl.work.ev_fork, side));
  {
    SwapStream sw(ctx, side);
    EcBase by, bY;
    by.enc = (const uint8_t*)dy; by.enc_stride = L;
    bY.enc = (const uint8_t*)dY; bY.enc_stride = L;
    RET_IF(ec_dual(ctx, gi, by, (const uint8_t*)dr, 32, &bY, dc, 0, n, w.tab1, w.tab2, w.p2, d2, ok + t, ok + t + n));
    HIPCHK(ctx, hipEventRecord(sl.work.ev_a2, ctx->stream));
    if (split_a1) {       // r G (the comb half of a1) now, beside the X path: what follows X is one table multiplication and an addition
      TIMED_LAUNCH(ctx, 1, ec_launch_dual_win(group, comb, nullptr, (const uint8_t*)dr, 32, nullptr, nullptr, 0, (int)n, (uint32_t*)w.pg.p,
                                              ctx->stream));
      HIPCHK(ctx, hipEventRecord(sl.work.ev_gr, ctx->stream));
    }
  }
  // X_i, then a1 = r*G + c*X_i   (participant.rs:1404-1417 / 1847-1860, dleq.rs:75-77)
  const int* gate;
  const uint32_t* xpts;
  if (pre) {       // X came from a batch launch: wait for it (the a2 side is already running), take the commitments' flags
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, pre->ready, 0));
    HIPCHK(ctx, hipMemcpyAsync(ok, pre->ok_cm, t, hipMemcpyDeviceToDevice, ctx->stream));
    dX = const_cast<uint8_t*>(pre->x_enc);
    xpts = pre->x_pts;
    gate = pre->gate;
  } else {
    RET_IF(ec_eval_x(ctx, gi, w, t, hpos, (const int64_t*)dpos_v, n, dX, &gate, &xpts));
  }
  if (split_a1) {
    TIMED_LAUNCH(ctx, 2, ec_launch_build_tables(group, dX, L, xpts, (int)n, (uint32_t*)w.tab3.p, nullptr, gate, ctx->stream));
    TIMED_LAUNCH(ctx, 1, ec_launch_dual_win(group, nullptr, nullptr, (const uint8_t*)dr, 32, (const uint32_t*)w.tab3.p, dc, 0, (int)n,
                                            (uint32_t*)w.p1.p, ctx->stream));                       // c X
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, sl.work.ev_gr, 0));
    LAUNCHCHK(ctx, ec_launch_add_pts(group, (const uint32_t*)w.p1.p, (const uint32_t*)w.pg.p, (int)n, (uint32_t*)w.p1.p, ctx->stream));
    TIMED_LAUNCH(ctx, 3, ec_launch_encode(group, (const uint32_t*)w.p1.p, (int)n, d1, ctx->stream));
  } else {
    EcBase bg, bX;
    bg.generator = true;
    bX.enc = dX; bX.enc_stride = L; bX.pts = xpts; bX.gate = gate;
    RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dr, 32, &bX, dc, 0, n, w.tab3, w.tab3, w.p1, d1, nullptr, nullptr));
  }
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, sl.work.ev_a2, 0));
  HIPCHK(ctx, hipMemcpyAsync(st.X, dX, n * L, hipMemcpyDeviceToHost, ctx->stream));
  if (space == MPVSS_HOST) memcpy(st.Y, shares, n * L);
  else HIPCHK(ctx, hipMemcpyAsync(st.Y, dY, n * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.a1, d1, n * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.a2, d2, n * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.ok, ok, okn, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.flags + 1, flags + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (gate != nullptr) HIPCHK(ctx, hipMemcpyAsync(st.flags, gate, 4, hipMemcpyDeviceToHost, ctx->stream));
  return be.commit();
}

int ec_verify_block_absorb_locked(mpvss_ctx* ctx, std::unique_lock<std::mutex>& lk, uint8_t* state, uint8_t* x_out,
                                  uint8_t* a1_out, uint8_t* a2_out, uint8_t* y_out, const unsigned long long* ticket, bool by_position) {
  if (!state) return fail(ctx, MPVSS_E_INVALID, "ec absorb: null transcript state");
  // the oldest block that waits for a FIFO consumer / the one mpvss_block_claim handed out / the caller's own (select_block)
  mpvss_ctx::BlockSlot* slp = select_block(ctx, ticket, by_position, 2, 2, "ec absorb");
  if (!slp) return MPVSS_E_INVALID;
  mpvss_ctx::BlockSlot& sl = *slp;
  const size_t n = sl.n, t = sl.t;
  const EcInfo* gi = ec_info(sl.group);
  const bool dealer = sl.dealer;
  const size_t L = gi->enc;
  const EcStaging st = ec_staging(sl.pin, n, t, L);
  long bad_elem = -1;
  const char* bad_what = "";
  Absorbed a;
  RET_IF(absorb_block(ctx, lk, sl, a, [&](bool done) {
    if (!done) return;
    for (size_t i = 0; i < t + 2 * n && bad_elem < 0; ++i)
      if (!st.ok[i]) {
        bad_elem = i < t ? (long)i : (long)((i - t) % n);
        bad_what = i < t ? "commitments" : (i < t + n ? "public keys" : "encrypted shares");
      }
    if (bad_elem < 0 && st.flags[1] == INT_MAX && (!sl.dealer || st.flags[2] == INT_MAX)) {
      mpvss::Sha256 tr;
      memcpy(&tr, state, sizeof(tr));
      ec_frame_shares(tr, st.X, st.Y, st.a1, st.a2, L, 0, n);      // dleq.rs:87-99, share order = array order
      memcpy(state, &tr, sizeof(tr));
      if (x_out) memcpy(x_out, st.X, n * L);
      if (y_out) memcpy(y_out, st.Y, n * L);
      if (a1_out) memcpy(a1_out, st.a1, n * L);
      if (a2_out) memcpy(a2_out, st.a2, n * L);
    }
  }));
  if (!a.waited) return MPVSS_OK;
  if (a.e != hipSuccess) return fail(ctx, MPVSS_E_DEVICE, "ec absorb: hipEventSynchronize", a.e);
  // the X path's device gate, as the MODP blocks count it (mpvss_fd_stats): 1 = the forward-difference pipelines held, 0 = the
  // gated Horner launch computed every X (a stage gave up, or device-resident positions were not consecutive); -1 = no gate
  if (!dealer && st.flags[0] != -1) {
    ++ctx->fd_blocks;
    if (st.flags[0] == 0) ++ctx->fd_fallbacks;
  }
  if (st.flags[1] != INT_MAX) return ec_report_bad_scalar(ctx, dealer ? "polynomial values" : "responses", (size_t)st.flags[1]);
  if (dealer && st.flags[2] != INT_MAX) return ec_report_bad_scalar(ctx, "witnesses", (size_t)st.flags[2]);
  if (bad_elem >= 0) return ec_report_bad_element(ctx, bad_what, (size_t)bad_elem);
  RET_IF(spans_sum(ctx, sl.spans, ctx->kernel_ms));
  pstats_add(ctx, sl, a, true, 1);
  return MPVSS_OK;
}

}  // namespace

namespace {
// Dealer side of distribute_secret for the curve groups (participant.rs:1094-1274, 1573-1717) as a block: the same slot
// kind, staging layout and absorbing hash as a verifier's block.  X_i from the commitments (the reference's loop) or --
// commitments == null -- as P(i) * G through the comb; Y_i = P(i) * y_i and a2_i = w_i * y_i share the table of y_i;
// a1_i = w_i * G.
// the dealer's polynomial for a block whose P(i) is computed on the device, on the block's own stream ahead of the group work
struct EcDealPoly {
  const uint8_t* coeffs_host;     // t x 32 bytes in the group's byte order (null when coeffs_dev is given)
  size_t t;
  const int64_t* positions_dev;   // n positions (`position as u64`, participant.rs:1419 / 1862)
  uint8_t* p_dev_out;             // n x 32 bytes: P(i) mod order, kept by the caller for the responses
  const uint8_t* coeffs_dev = nullptr;
};

int ec_distribute_compute_locked(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                 const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values,
                                 const uint8_t* witnesses, size_t n, uint8_t* x_dev_out, uint8_t* y_dev_out,
                                 uint8_t* a1_dev_out, uint8_t* a2_dev_out, const EcDealPoly* poly = nullptr,
                                 const mpvss_ec_keyset* keyset = nullptr, size_t key_offset = 0) {
  const EcInfo* gi = ec_info(group);
  if (!gi) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_distribute: unknown group");
  // keyset != null: the keys key_offset .. key_offset + n - 1 of the set stand for pubkeys (admitted by the caller): Y and a2 by
  // one walk over their rows -- no key staging, decode or table build
  if (keyset && space != MPVSS_DEVICE) return fail(ctx, MPVSS_E_INVALID, "ec_distribute: a key set takes device buffers");
  if (poly) {
    if (space != MPVSS_DEVICE || commitments || (!poly->coeffs_host && !poly->coeffs_dev) || !poly->positions_dev || !poly->p_dev_out ||
        poly->t == 0 || poly->t > 0x7fffffff)
      return fail(ctx, MPVSS_E_INVALID, "ec_deal: bad argument (device buffers, t >= 1)");
    p_values = poly->p_dev_out;
  }
  if (n > 0 && ((!pubkeys && !keyset) || !p_values || !witnesses || n > 0x7fffffff ||
                (commitments && (!positions || t == 0 || t > 0x7fffffff))))
    return fail(ctx, MPVSS_E_INVALID, "ec_distribute: bad argument");
  if (!commitments) t = 0;      // (threshold > n is the whole box's business -- mpvss_ec_distribute checks it; a block may be smaller)
  BlockEnqueue be(ctx, 2, n, "ec_distribute");
  RET_IF(be.rc);
  mpvss_ctx::BlockSlot& sl = be.sl;
  sl.dealer = true;
  sl.group = group;
  sl.t = t;
  if (n == 0) return be.commit_empty();
  const uint32_t* comb;
  RET_IF(ec_comb(ctx, group, &comb));
  RET_IF(be.enter());
  EcWork& w = sl.ecw;
  const size_t L = gi->enc;
  RET_IF(be.pin(ec_staging_out_bytes(n, t, L) + (space == MPVSS_HOST ? n * L + 2 * n * 32 + t * L + n * 8 : 0) +
                (poly && !poly->coeffs_dev ? poly->t * 32 : 0)));
  EcStaging st = ec_staging(sl.pin, n, t, L);
  if (poly) {
    // P(i) mod order first, on this block's own stream: the group work below reads it in stream order
    const size_t cb = poly->t * 32;
    RET_IF(ensure(ctx, w.c, cb + poly->t * 32));                    // coefficient bytes | their Montgomery forms
    const uint8_t* dc = poly->coeffs_dev;
    uint8_t* hc = st.in;
    if (!dc) {
      memcpy(hc, poly->coeffs_host, cb);
      HIPCHK(ctx, hipMemcpyAsync(w.c.p, hc, cb, hipMemcpyHostToDevice, ctx->stream));
      dc = (const uint8_t*)w.c.p;
    }
    LAUNCHCHK(ctx, ec_scalar_launch_poly_eval(group, dc, (int)poly->t, poly->positions_dev, (int)n, (uint32_t*)((uint8_t*)w.c.p + cb),
                                              poly->p_dev_out, ctx->stream));
    // the coefficients are the dealer's secret: zero the device copies and, in stream order, the pinned one
    HIPCHK(ctx, hipMemsetAsync(w.c.p, 0, 2 * cb, ctx->stream));
    if (!poly->coeffs_dev) HIPCHK(ctx, hipMemcpyAsync(hc, w.c.p, cb, hipMemcpyDeviceToHost, ctx->stream));
  }
  const int64_t* hpos = nullptr;
  if (space == MPVSS_HOST) {
    uint8_t* in = st.in;
    memcpy(in, pubkeys, n * L); pubkeys = in; in += n * L;
    memcpy(in, p_values, n * 32); p_values = in; in += n * 32;
    memcpy(in, witnesses, n * 32); witnesses = in; in += n * 32;
    if (commitments) {
      memcpy(in, commitments, t * L); commitments = in; in += t * L;
      memcpy(in, positions, n * 8); positions = (const int64_t*)in;
      hpos = positions;
    }
  }
  const size_t okn = t + 2 * n;
  RET_IF(ensure(ctx, w.ok, okn));
  RET_IF(ensure(ctx, w.flags, 64));
  uint8_t* ok = (uint8_t*)w.ok.p;
  int* flags = (int*)w.flags.p;
  st.flags[0] = -1;
  st.flags[1] = st.flags[2] = INT_MAX;
  HIPCHK(ctx, hipMemcpyAsync(flags + 1, st.flags + 1, 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ok, 1, okn, ctx->stream));          // the flags nobody writes here count as valid
  if (commitments) RET_IF(ec_stage_commitments_async(ctx, gi, w, space, commitments, t, ok));
  const void *dy = nullptr, *dp, *dw;
  if (!keyset) RET_IF(stage_in(ctx, space, pubkeys, n * L, w.a, &dy));
  RET_IF(stage_in(ctx, space, p_values, n * 32, w.d, &dp));
  RET_IF(stage_in(ctx, space, witnesses, n * 32, w.e, &dw));
  LAUNCHCHK(ctx, verdict_launch_check_scalars(group, (const uint8_t*)dp, (int)n, flags + 1, ctx->stream));
  LAUNCHCHK(ctx, verdict_launch_check_scalars(group, (const uint8_t*)dw, (int)n, flags + 2, ctx->stream));
  RET_IF(ensure(ctx, w.x, n * L));
  RET_IF(ensure(ctx, w.b, n * L));
  RET_IF(ensure(ctx, w.o1, n * L));
  RET_IF(ensure(ctx, w.o2, n * L));
  uint8_t *dX = (uint8_t*)w.x.p, *dY = (uint8_t*)w.b.p, *d1 = (uint8_t*)w.o1.p, *d2 = (uint8_t*)w.o2.p;
  EcBase by, bg;
  by.enc = (const uint8_t*)dy; by.enc_stride = L;
  bg.generator = true;
  const int* gate = nullptr;
  if (commitments) {
    const void* dpos_v;
    RET_IF(stage_in(ctx, space, positions, n * 8, w.pos, &dpos_v));
    const uint32_t* xpts;
    RET_IF(ec_eval_x(ctx, gi, w, t, hpos, (const int64_t*)dpos_v, n, dX, &gate, &xpts));
  } else {
    RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dp, 32, nullptr, nullptr, 0, n, w.tab2, w.tab2, w.p1, dX, nullptr, nullptr));   // X = p * G
  }
  if (keyset) {
    // Y = p * y and a2 = w * y from the rows of y_i: one walk, two encodes (the key flags count as valid: create checked the keys)
    const size_t pts_bytes = n * (size_t)ec_point_words(group) * 4;
    RET_IF(ensure(ctx, w.p1, pts_bytes));
    RET_IF(ensure(ctx, w.p2, pts_bytes));
    RET_IF(ec_keyset_walk(ctx, keyset, key_offset, (const uint8_t*)dp, (const uint8_t*)dw, n, (uint32_t*)w.p1.p, (uint32_t*)w.p2.p));
    TIMED_LAUNCH(ctx, 3, ec_launch_encode(group, (const uint32_t*)w.p1.p, (int)n, dY, ctx->stream));
    TIMED_LAUNCH(ctx, 3, ec_launch_encode(group, (const uint32_t*)w.p2.p, (int)n, d2, ctx->stream));
    RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dw, 32, nullptr, nullptr, 0, n, w.tab2, w.tab2, w.p1, d1, nullptr, nullptr));   // a1 = w * G
  } else {
    // the table of y_i serves both Y = p * y (participant.rs:1190) and a2 = w * y (dleq.rs:214-216)
    RET_IF(ec_dual(ctx, gi, by, (const uint8_t*)dp, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p1, dY, ok + t, nullptr));
    RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dw, 32, nullptr, nullptr, 0, n, w.tab2, w.tab2, w.p1, d1, nullptr, nullptr));   // a1 = w * G
    by.table = (const uint32_t*)w.tab1.p;
    RET_IF(ec_dual(ctx, gi, by, (const uint8_t*)dw, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p2, d2, nullptr, nullptr));   // a2 = w * y
  }
  HIPCHK(ctx, hipMemcpyAsync(st.X, dX, n * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.Y, dY, n * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.a1, d1, n * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.a2, d2, n * L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.ok, ok, okn, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(st.flags + 1, flags + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (gate != nullptr) HIPCHK(ctx, hipMemcpyAsync(st.flags, gate, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (space == MPVSS_DEVICE) {
    if (x_dev_out) HIPCHK(ctx, hipMemcpyAsync(x_dev_out, dX, n * L, hipMemcpyDeviceToDevice, ctx->stream));
    if (y_dev_out) HIPCHK(ctx, hipMemcpyAsync(y_dev_out, dY, n * L, hipMemcpyDeviceToDevice, ctx->stream));
    if (a1_dev_out) HIPCHK(ctx, hipMemcpyAsync(a1_dev_out, d1, n * L, hipMemcpyDeviceToDevice, ctx->stream));
    if (a2_dev_out) HIPCHK(ctx, hipMemcpyAsync(a2_dev_out, d2, n * L, hipMemcpyDeviceToDevice, ctx->stream));
  }
  return be.commit();
}
}  // namespace

extern "C" int mpvss_ec_distribute_compute(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                           const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values,
                                           const uint8_t* witnesses, size_t n, uint8_t* x_dev_out, uint8_t* y_dev_out,
                                           uint8_t* a1_dev_out, uint8_t* a2_dev_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ec_distribute_compute_locked(ctx, group, space, commitments, t, positions, pubkeys, p_values, witnesses, n, x_dev_out,
                                      y_dev_out, a1_dev_out, a2_dev_out);
}
extern "C" int mpvss_ec_distribute_absorb(mpvss_ctx* ctx, uint8_t* state, uint8_t* x_out_host, uint8_t* y_out_host,
                                          uint8_t* a1_out_host, uint8_t* a2_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  return ec_verify_block_absorb_locked(ctx, lk, state, x_out_host, a1_out_host, a2_out_host, y_out_host);
}

// ---- the curve groups' dealer with the scalar side on the device as well (participant.rs:1134-1168, 1200-1230, 1607-1631) ------
// (mpvss_ec_poly_eval_device / mpvss_ec_dleq_responses_device: capi_scalar.inc, beside their MODP counterparts)
extern "C" int mpvss_ec_deal_compute(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                                     const uint8_t* pubkeys_dev, const uint8_t* witnesses_dev, size_t n, uint8_t* p_dev_out,
                                     uint8_t* x_dev_out, uint8_t* y_dev_out, uint8_t* a1_dev_out, uint8_t* a2_dev_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return fail(ctx, MPVSS_E_INVALID, "ec_deal_compute: no shares");
  const EcDealPoly poly{coeffs_host, t, positions_dev, p_dev_out};
  return ec_distribute_compute_locked(ctx, group, MPVSS_DEVICE, nullptr, 0, nullptr, pubkeys_dev, p_dev_out, witnesses_dev, n, x_dev_out,
                                      y_dev_out, a1_dev_out, a2_dev_out, &poly);
}

// The dealer of participant.rs:1094-1274 / 1573-1717 in ONE call from host buffers: P(i), X_i = P(i) G, Y_i = P(i) y_i, a1, a2,
// the transcript digest, the challenge c = hash_to_scalar(digest) and the responses r_i = w_i - P(i) c.  Inputs and
// intermediate secrets in the deal's own buffers (a set per deal in flight from the context's pool), P(i) and the witnesses zeroed at the end.
// The keys: a host array (mpvss_ec_deal), or the keys key_offset .. of a key set admitted by the caller (mpvss_ec_deal_keyset: no
// key upload).  Context lock held on entry and on return.
namespace {
int ec_deal_locked(mpvss_ctx* ctx, std::unique_lock<std::mutex>& lk, int group, const uint8_t* coeffs_host, size_t t,
                   const int64_t* positions_host, const uint8_t* pubkeys_host, const mpvss_ec_keyset* keyset, size_t key_offset,
                   const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out, uint8_t* a2_out,
                   uint8_t* digest32_out, uint8_t* challenge_out32, uint8_t* r_out) {
  const EcInfo* gi = ec_info(group);
  if (!gi) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_deal: unknown group");
  if (n == 0 || !coeffs_host || !positions_host || (!pubkeys_host && !keyset) || !witnesses_host || !y_out || !r_out || t == 0 ||
      t > 0x7fffffff || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "ec_deal: bad argument (t >= 1, 1 <= n < 2^31)");
  if (t > n) return fail(ctx, MPVSS_E_INVALID, "ec_deal: threshold > number of public keys (participant.rs:1100)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t L = gi->enc;
  mpvss_ctx::DealBufs* dbufs = ctx->deal_acquire();        // (one set per deal in flight: several threads may deal on one context)
  if (!dbufs) return fail(ctx, MPVSS_E_NOMEM, "ec_deal: no buffers");
  mpvss_ctx::DealBufs& d = *dbufs;
  struct Wipe {
    mpvss_ctx* c; mpvss_ctx::DealBufs* dp; size_t n, t;
    ~Wipe() {
      mpvss_ctx::DealBufs& d = *dp;
      if (hipSetDevice(c->device) == hipSuccess) {
        if (d.p.p) (void)hipMemsetAsync(d.p.p, 0, std::min(d.p.cap, n * 32), c->stream);
        if (d.w.p) (void)hipMemsetAsync(d.w.p, 0, std::min(d.w.cap, n * 32), c->stream);
        if (d.coef.p) (void)hipMemsetAsync(d.coef.p, 0, std::min(d.coef.cap, t * 32), c->stream);
        (void)hipStreamSynchronize(c->stream);
      }
      d.in_use = false;
    }
  } wipe{ctx, dbufs, n, t};
  static const int trace_deal = fd_env("MPVSS_TRACE_DEAL", 0);
  const auto t_d0 = std::chrono::steady_clock::now();
  double t_marks[4] = {0, 0, 0, 0};
  auto dmark = [&](int k) { t_marks[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_d0).count(); };
  if (!keyset) RET_IF(ensure(ctx, d.keys, n * L));
  for (DevBuf* b : {&d.p, &d.w, &d.r}) RET_IF(ensure(ctx, *b, n * 32));
  RET_IF(ensure(ctx, d.pos, n * 8));
  RET_IF(ensure(ctx, d.coef, t * 32));
  RET_IF(ensure(ctx, d.c, 32));
  HIPCHK(ctx, hipMemcpyAsync(d.coef.p, coeffs_host, t * 32, hipMemcpyHostToDevice, ctx->stream));
  if (!keyset) HIPCHK(ctx, hipMemcpyAsync(d.keys.p, pubkeys_host, n * L, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d.w.p, witnesses_host, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d.pos.p, positions_host, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // the block's own streams read them next
  dmark(0);
  const EcDealPoly poly{nullptr, t, (const int64_t*)d.pos.p, (uint8_t*)d.p.p, (const uint8_t*)d.coef.p};
  RET_IF(wait_for_room(ctx, lk));
  RET_IF(ec_distribute_compute_locked(ctx, group, MPVSS_DEVICE, nullptr, 0, nullptr, keyset ? nullptr : (const uint8_t*)d.keys.p,
                                      (const uint8_t*)d.p.p, (const uint8_t*)d.w.p, n, nullptr, nullptr, nullptr, nullptr, &poly, keyset,
                                      key_offset));
  const unsigned long long blk = ctx->own_last(1);
  dmark(1);
  uint8_t state[MPVSS_TRANSCRIPT_STATE_BYTES];
  mpvss_transcript_init(state);
  RET_IF(ec_verify_block_absorb_locked(ctx, lk, state, x_out, a1_out, a2_out, y_out, &blk, true));
  dmark(2);
  uint8_t digest[32], challenge[32];
  {
    mpvss::Sha256 tr;
    memcpy(&tr, state, sizeof(tr));
    tr.final(digest);
  }
  ec_hash_to_scalar_bytes(gi, digest, 32, challenge);       // participant.rs:1200-1210 / 1662-1672
  if (digest32_out) memcpy(digest32_out, digest, 32);
  if (challenge_out32) memcpy(challenge_out32, challenge, 32);
  HIPCHK(ctx, hipMemcpy(d.c.p, challenge, 32, hipMemcpyHostToDevice));
  LAUNCHCHK(ctx, ec_scalar_launch_responses(group, (const uint8_t*)d.w.p, (const uint8_t*)d.p.p, (const uint8_t*)d.c.p, 0, (int)n,
                                            (uint8_t*)d.r.p, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(r_out, d.r.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  dmark(3);
  if (trace_deal)
    fprintf(stderr, "[mpvss] ec_deal group=%d n=%zu t=%zu: staging %.1f | enqueue %.1f | wait + hash + copies %.1f | challenge + responses + copy %.1f ms "
            "(pipeline: wait %.1f, hash %.1f)\n", group, n, t, t_marks[0], t_marks[1] - t_marks[0], t_marks[2] - t_marks[1], t_marks[3] - t_marks[2],
            ctx->pstats.wait_ms, ctx->pstats.hash_ms);
  return MPVSS_OK;
}
}  // namespace

extern "C" int mpvss_ec_deal(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                             const uint8_t* pubkeys_host, const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out,
                             uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out32, uint8_t* r_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  return ec_deal_locked(ctx, lk, group, coeffs_host, t, positions_host, pubkeys_host, nullptr, 0, witnesses_host, n, x_out, y_out, a1_out,
                        a2_out, digest32_out, challenge_out32, r_out);
}

// =====================================================================================================================
// Key sets of a curve group (DESIGN section 13, "Key sets, curve groups"): the per-key combs of long-lived public keys, built
// once, and the calls that multiply those keys over them -- Y_i = P(i) y_i and a2_i = w_i y_i of the dealer, and the stand-alone
// multiples.  A set is explicit: the caller built it and names it, so nothing here decides by a threshold.
// =====================================================================================================================
extern "C" size_t mpvss_ec_keyset_bytes_per_key(int group) {
  return ec_info(group) ? ec_keyset_row_words(group) * 4 + EC_KEYSET_MARK_BYTES : 0;
}

extern "C" size_t mpvss_ec_keyset_bytes(const mpvss_ec_keyset* ks) {
  return ks ? ks->n * (ec_keyset_row_words(ks->group) * 4 + EC_KEYSET_MARK_BYTES) : 0;
}

extern "C" int mpvss_ec_keyset_create(mpvss_ctx* ctx, int group, int space, const uint8_t* pubkeys, size_t n, mpvss_ec_keyset** out) {
  if (out) *out = nullptr;
  EC_PROLOGUE("ec_keyset_create");
  if (!out || !pubkeys || n == 0 || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_keyset_create: bad argument (n >= 1)");
  mpvss_ec_keyset* ks = new (std::nothrow) mpvss_ec_keyset();
  if (!ks) return fail(ctx, MPVSS_E_NOMEM, "ec_keyset_create: no memory for the handle");
  ks->ctx = ctx;
  ks->group = group;
  ks->n = n;
  const int rc = [&]() -> int {
    const size_t row_words = ec_keyset_row_words(group);
    hipError_t e = hipMalloc((void**)&ks->rows, n * row_words * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&ks->marks, n * EC_KEYSET_MARK_BYTES);
    if (e != hipSuccess) {
      (void)hipGetLastError();       // the runtime's last-error slot is sticky: the next launcher must not see this
      return fail(ctx, MPVSS_E_NOMEM, "ec_keyset_create: hipMalloc(rows)", e);
    }
    // a chunk's launches work on at most 2^16 keys (and never more than MPVSS_MAX_CHUNK): keys x 65 windows fits the
    // launcher's int with room, and the staging buffer of host keys stays at 2 MB
    const size_t step = std::min(MAX_CHUNK, (size_t)1 << 16);
    RET_IF(ensure(ctx, w.ok, std::max(step, (size_t)4096)));
    std::vector<uint8_t> okh(std::min(step, n));
    for (size_t off = 0; off < n; off += step) {
      const size_t cnt = std::min(n - off, step);
      const void* dk;
      RET_IF(stage_in(ctx, space, pubkeys + off * gi->enc, cnt * gi->enc, w.a, &dk));
      TIMED_LAUNCH(ctx, 2, ec_launch_keyset_build(group, (const uint8_t*)dk, (int)cnt, ks->rows + off * row_words, (uint8_t*)w.ok.p,
                                                  ks->marks + off, ctx->stream));
      // the chunk's validity flags; the wait also frees the staging buffer for the next chunk
      HIPCHK(ctx, hipMemcpyAsync(okh.data(), w.ok.p, cnt, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      for (size_t i = 0; i < cnt; ++i)
        if (!okh[i]) return ec_report_bad_element(ctx, "ec_keyset_create: public keys", off + i);      // chunks in order: the smallest bad index
    }
    return spans_collect(ctx);
  }();
  if (rc != MPVSS_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    if (ks->rows) (void)hipFree(ks->rows);
    if (ks->marks) (void)hipFree(ks->marks);
    delete ks;
    return rc;
  }
  ctx->ec_ks_keys_built += n;
  *out = ks;
  return MPVSS_OK;
}

// A block enqueued by mpvss_ec_deal_compute_keyset may still read the rows: every stream of the set's context is drained first.
extern "C" void mpvss_ec_keyset_destroy(mpvss_ctx* ctx, mpvss_ec_keyset* ks) {
  if (!ks) return;
  mpvss_ctx* const owner = ks->ctx;          // the set is freed on its own context's device whichever context is named
  (void)ctx;
  (void)mpvss_ctx_synchronize(owner);
  std::lock_guard<std::mutex> lk(owner->mu);
  if (hipSetDevice(owner->device) == hipSuccess) {
    if (ks->rows) (void)hipFree(ks->rows);
    if (ks->marks) (void)hipFree(ks->marks);
  }
  delete ks;
}

extern "C" int mpvss_ec_keyset_stats(mpvss_ctx* ctx, unsigned long long* keys_built, unsigned long long* powers_from_rows) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (keys_built) *keys_built = ctx->ec_ks_keys_built;
  if (powers_from_rows) *powers_from_rows = ctx->ec_ks_powers;
  return MPVSS_OK;
}

extern "C" int mpvss_ec_keyset_twin_exp(mpvss_ctx* ctx, int group, int space, const mpvss_ec_keyset* keyset, size_t key_offset,
                                        const uint8_t* e1, const uint8_t* e2, size_t n, uint8_t* out1, uint8_t* out2) {
  EC_PROLOGUE("ec_keyset_twin_exp");
  if (const char* why = ec_keyset_refusal(ctx, group, keyset, key_offset, n)) return fail(ctx, MPVSS_E_INVALID, why);
  if (n == 0) return MPVSS_OK;
  if (!e1 || !out1 || (e2 == nullptr) != (out2 == nullptr) || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "ec_keyset_twin_exp: bad argument (e2 and out2 are given together)");
  RET_IF(ec_check_scalars(ctx, gi, space, e1, n, "ec_keyset_twin_exp e1"));
  if (e2) RET_IF(ec_check_scalars(ctx, gi, space, e2, n, "ec_keyset_twin_exp e2"));
  const size_t L = gi->enc, pw = (size_t)ec_point_words(group);
  // chunks of at most MPVSS_MAX_CHUNK shares, as the run-time groups' calls chunk: the workspace stays bounded whatever n is
  const size_t step = MAX_CHUNK;
  for (size_t off = 0; off < n; off += step) {
    const size_t cnt = std::min(n - off, step);
    const void *d1, *d2 = nullptr;
    RET_IF(stage_in(ctx, space, e1 + off * 32, cnt * 32, w.d, &d1));
    if (e2) RET_IF(stage_in(ctx, space, e2 + off * 32, cnt * 32, w.e, &d2));
    uint8_t *o1 = out1 + off * L, *o2 = e2 ? out2 + off * L : nullptr;
    if (space == MPVSS_HOST) {
      RET_IF(ensure(ctx, w.o1, cnt * L)); o1 = (uint8_t*)w.o1.p;
      if (e2) { RET_IF(ensure(ctx, w.o2, cnt * L)); o2 = (uint8_t*)w.o2.p; }
    }
    RET_IF(ensure(ctx, w.p1, cnt * pw * 4));
    if (e2) RET_IF(ensure(ctx, w.p2, cnt * pw * 4));
    RET_IF(ec_keyset_walk(ctx, keyset, key_offset + off, (const uint8_t*)d1, (const uint8_t*)d2, cnt, (uint32_t*)w.p1.p,
                          e2 ? (uint32_t*)w.p2.p : nullptr));
    TIMED_LAUNCH(ctx, 3, ec_launch_encode(group, (const uint32_t*)w.p1.p, (int)cnt, o1, ctx->stream));
    if (e2) TIMED_LAUNCH(ctx, 3, ec_launch_encode(group, (const uint32_t*)w.p2.p, (int)cnt, o2, ctx->stream));
    if (space == MPVSS_HOST) {
      RET_IF(copy_out(ctx, space, out1 + off * L, o1, cnt * L));
      if (e2) RET_IF(copy_out(ctx, space, out2 + off * L, o2, cnt * L));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // the staging buffers are reused by the next chunk
  }
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

extern "C" int mpvss_ec_keyset_dual_exp(mpvss_ctx* ctx, int group, int space, const mpvss_ec_keyset* keyset, size_t key_offset,
                                        const uint8_t* e1, const uint8_t* h2, const uint8_t* e2, int e2_per_share, size_t n,
                                        uint8_t* out) {
  EC_PROLOGUE("ec_keyset_dual_exp");
  if (const char* why = ec_keyset_refusal(ctx, group, keyset, key_offset, n)) return fail(ctx, MPVSS_E_INVALID, why);
  if (n == 0) return MPVSS_OK;
  if (!e1 || !out || (h2 && !e2) || n > 0x7fffffff) return fail(ctx, MPVSS_E_INVALID, "ec_keyset_dual_exp: bad argument");
  RET_IF(ec_check_scalars(ctx, gi, space, e1, n, "ec_keyset_dual_exp e1"));
  if (h2) RET_IF(ec_check_scalars(ctx, gi, e2_per_share ? space : MPVSS_HOST, e2, e2_per_share ? n : 1, "ec_keyset_dual_exp e2"));
  const size_t L = gi->enc, pw = (size_t)ec_point_words(group);
  const void* dshared = nullptr;
  if (h2 && !e2_per_share) RET_IF(stage_in(ctx, MPVSS_HOST, e2, 32, w.chal, &dshared));      // host bytes, as c of ec_dleq_commitments
  const size_t step = MAX_CHUNK;
  RET_IF(ensure(ctx, w.ok, std::max(std::min(n, step), (size_t)4096)));
  for (size_t off = 0; off < n; off += step) {
    const size_t cnt = std::min(n - off, step);
    const void *d1, *dh = nullptr, *d2 = dshared;
    RET_IF(stage_in(ctx, space, e1 + off * 32, cnt * 32, w.d, &d1));
    if (h2) RET_IF(stage_in(ctx, space, h2 + off * L, cnt * L, w.c, &dh));
    if (h2 && e2_per_share) RET_IF(stage_in(ctx, space, e2 + off * 32, cnt * 32, w.e, &d2));
    uint8_t* o = out + off * L;
    if (space == MPVSS_HOST) { RET_IF(ensure(ctx, w.o1, cnt * L)); o = (uint8_t*)w.o1.p; }
    RET_IF(ensure(ctx, w.p1, cnt * pw * 4));
    RET_IF(ec_keyset_walk(ctx, keyset, key_offset + off, (const uint8_t*)d1, nullptr, cnt, (uint32_t*)w.p1.p, nullptr));
    if (h2) {
      // e2 * h2 by the one-table window kernel (the result stays in internal coordinates), then one addition
      EcBase bh;
      bh.enc = (const uint8_t*)dh;
      bh.enc_stride = L;
      RET_IF(ec_dual(ctx, gi, bh, (const uint8_t*)d2, e2_per_share ? 32 : 0, nullptr, nullptr, 0, cnt, w.tab1, w.tab2, w.p2, nullptr,
                     (uint8_t*)w.ok.p, nullptr));
      LAUNCHCHK(ctx, ec_launch_add_pts(group, (const uint32_t*)w.p1.p, (const uint32_t*)w.p2.p, (int)cnt, (uint32_t*)w.p1.p, ctx->stream));
    }
    TIMED_LAUNCH(ctx, 3, ec_launch_encode(group, (const uint32_t*)w.p1.p, (int)cnt, o, ctx->stream));
    if (space == MPVSS_HOST) RET_IF(copy_out(ctx, space, out + off * L, o, cnt * L));
    if (h2) {
      std::vector<uint8_t> okh(cnt);
      HIPCHK(ctx, hipMemcpyAsync(okh.data(), w.ok.p, cnt, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      for (size_t i = 0; i < cnt; ++i)
        if (!okh[i]) return ec_report_bad_element(ctx, "ec_keyset_dual_exp h2", off + i);
    } else {
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // the staging buffers are reused by the next chunk
    }
  }
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}

extern "C" int mpvss_ec_deal_compute_keyset(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                                            const mpvss_ec_keyset* keyset, size_t key_offset, const uint8_t* witnesses_dev, size_t n,
                                            uint8_t* p_dev_out, uint8_t* x_dev_out, uint8_t* y_dev_out, uint8_t* a1_dev_out,
                                            uint8_t* a2_dev_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ec_info(group)) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_deal_compute_keyset: unknown group");
  if (const char* why = ec_keyset_refusal(ctx, group, keyset, key_offset, n)) return fail(ctx, MPVSS_E_INVALID, why);
  if (n == 0) return fail(ctx, MPVSS_E_INVALID, "ec_deal_compute_keyset: no shares");
  const EcDealPoly poly{coeffs_host, t, positions_dev, p_dev_out};
  return ec_distribute_compute_locked(ctx, group, MPVSS_DEVICE, nullptr, 0, nullptr, nullptr, p_dev_out, witnesses_dev, n, x_dev_out,
                                      y_dev_out, a1_dev_out, a2_dev_out, &poly, keyset, key_offset);
}

extern "C" int mpvss_ec_deal_keyset(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                                    const mpvss_ec_keyset* keyset, size_t key_offset, const uint8_t* witnesses_host, size_t n,
                                    uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out,
                                    uint8_t* challenge_out32, uint8_t* r_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  if (!ec_info(group)) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_deal_keyset: unknown group");
  if (const char* why = ec_keyset_refusal(ctx, group, keyset, key_offset, n)) return fail(ctx, MPVSS_E_INVALID, why);
  return ec_deal_locked(ctx, lk, group, coeffs_host, t, positions_host, nullptr, keyset, key_offset, witnesses_host, n, x_out, y_out, a1_out,
                        a2_out, digest32_out, challenge_out32, r_out);
}

// a block of a curve group taken by mpvss_block_claim (several threads absorb -- wait for and hash -- blocks side by side and each
// knows which block it holds): the verifier's and the dealer's blocks alike
extern "C" int mpvss_ec_block_absorb_claimed(mpvss_ctx* ctx, unsigned long long ticket, uint8_t* state, uint8_t* x_out_host,
                                             uint8_t* y_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  return ec_verify_block_absorb_locked(ctx, lk, state, x_out_host, a1_out_host, a2_out_host, y_out_host, &ticket, false);
}

extern "C" int mpvss_ec_verify_block_compute(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                             const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                             const uint8_t* responses, size_t n, const uint8_t* challenge_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ec_verify_block_compute_locked(ctx, group, space, commitments, t, positions, pubkeys, shares, responses, n,
                                        challenge_host);
}

extern "C" int mpvss_ec_verify_block_absorb(mpvss_ctx* ctx, uint8_t* state, uint8_t* x_out_host, uint8_t* a1_out_host,
                                            uint8_t* a2_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  return ec_verify_block_absorb_locked(ctx, lk, state, x_out_host, a1_out_host, a2_out_host, nullptr, nullptr, false);
}

// Host-only: extend the transcript with `count` encoded elements (framed, dleq.rs:58-61) / finish it
extern "C" int mpvss_ec_transcript_absorb(int group, uint8_t* state, const uint8_t* elements, size_t count) {
  const EcInfo* gi = ec_info(group);
  if (!gi || !state || (count && !elements)) return MPVSS_E_INVALID;
  mpvss::Sha256 tr;
  memcpy(&tr, state, sizeof(tr));
  for (size_t i = 0; i < count; ++i) ec_frame_update(tr, elements + i * gi->enc, gi->enc);
  memcpy(state, &tr, sizeof(tr));
  return MPVSS_OK;
}

extern "C" int mpvss_ec_transcript_verdict(int group, const uint8_t* state, const uint8_t* challenge_host, int* verdict,
                                           uint8_t* digest32_out) {
  const EcInfo* gi = ec_info(group);
  if (!gi || !state || !challenge_host || !verdict) return MPVSS_E_INVALID;
  mpvss::Sha256 tr;
  memcpy(&tr, state, sizeof(tr));
  uint8_t digest[32], hs[32];
  tr.final(digest);
  if (digest32_out) memcpy(digest32_out, digest, 32);
  ec_hash_to_scalar(gi, digest, hs);
  *verdict = memcmp(hs, challenge_host, 32) == 0 ? 1 : 0;      // participant.rs:1436-1441, 1879-1884
  return MPVSS_OK;
}

extern "C" int mpvss_ec_verify_distribution(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                            const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                            const uint8_t* responses, size_t n, const uint8_t* challenge_host,
                                            int* verdict, uint8_t* digest32_out, uint8_t* x_out_host,
                                            uint8_t* a1_out_host, uint8_t* a2_out_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  if (!ec_info(group)) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_verify_distribution: unknown group");
  if (!verdict || !challenge_host) return fail(ctx, MPVSS_E_INVALID, "ec_verify_distribution: bad argument");
  *verdict = 0;
  uint8_t state[MPVSS_TRANSCRIPT_STATE_BYTES];
  mpvss_transcript_init(state);
  RET_IF(wait_for_room(ctx, lk));
  RET_IF(ec_verify_block_compute_locked(ctx, group, space, commitments, t, positions, pubkeys, shares, responses, n,
                                        challenge_host));
  const unsigned long long blk = ctx->own_last(1);
  RET_IF(ec_verify_block_absorb_locked(ctx, lk, state, x_out_host, a1_out_host, a2_out_host, nullptr, &blk, true));
  return mpvss_ec_transcript_verdict(group, state, challenge_host, verdict, digest32_out);
}

// =====================================================================================================================
// Runs of small boxes as one dense batch (DESIGN section 8, "Runs of small boxes"): a verifier of a PVSS round holds one box per
// dealer, tens to hundreds of boxes of 5 to 1 000 shares.  Through a block slot each costs its own decode, Horner launch, three
// table builds, two or three multiplications, an addition and two encodes, about ten copies, two forks and an event wait: the
// latency of a chain of narrow launches.  A run of such boxes travels instead as ONE concatenation through the launches of one
// box, X by k_*_commit_eval_tiles (a tile = up to 64 shares of one box = one workgroup) and the DLEQ multiplications with a
// challenge per share.  Which boxes travel together: many::walk (host_many.h), called by mpvss_ec_verify_many below.
// =====================================================================================================================
namespace {

// A box of n or t >= 4096 never travels in a run: 4096 is the bound below which ec_fd_shape never holds, so no box that the
// forward differences or the X batches serve changes its path.  Derived, not measured.
constexpr size_t EC_GROUP_BOX_MAX = 4096;
constexpr size_t EC_TILE = 64;                     // shares per tile: one wave, one workgroup of the 64-lane curve kernels

// may this box travel in a run?  Judged on the host before anything is launched.
bool ec_box_small(const EcInfo* gi, const mpvss_ec_box& b) {
  if (b.n < 1 || b.n >= EC_GROUP_BOX_MAX || b.t < 1 || b.t >= EC_GROUP_BOX_MAX || b.n > MAX_CHUNK || b.t > MAX_CHUNK) return false;
  if (!b.commitments || !b.positions || !b.pubkeys || !b.shares || !b.responses || !b.challenge_host) return false;
  return scalar_canonical(gi, b.challenge_host);
}

// A grouped pass: the boxes [lo, hi) (all ec_box_small, at least two, at most MAX_CHUNK shares and as many commitments in all).
// Synchronous, under the context lock, on the context's own EcWork and pinned staging -- the lock is held for the pass (a few
// milliseconds); pipe_mu plays no part.  A box the engine turns down (an encoding that is no group element, a response that is
// not below the order) is refused here: its lanes ran with the others and are dropped.
int ec_many_run(mpvss_ctx* ctx, const EcInfo* gi, int space, const mpvss_ec_box* boxes, size_t lo, size_t hi, int hash_threads,
                int* verdicts, uint8_t* digests32) {
  const int group = gi->group;
  const size_t B = hi - lo, L = gi->enc, pw = (size_t)ec_point_words(group);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  EcWork& w = ecw(ctx);
  // the tables: tiles {box, first share, live count}, boxes {first commitment, t} (also the commitments' gather segments),
  // shares {first share, n} (the gather segments of the per-share arrays)
  std::vector<uint32_t> tab;
  std::vector<size_t> first(B + 1), first_cm(B + 1), counts(B);
  size_t S = 0, T = 0;
  for (size_t k = 0; k < B; ++k) {
    const mpvss_ec_box& b = boxes[lo + k];
    first[k] = S;
    first_cm[k] = T;
    counts[k] = b.n;
    S += b.n;
    T += b.t;
  }
  first[B] = S;
  first_cm[B] = T;
  many::tile_table(counts.data(), B, EC_TILE, 3, tab);
  const size_t ntiles = tab.size() / 3;
  const size_t o_btab = tab.size();
  for (size_t k = 0; k < B; ++k) { tab.push_back((uint32_t)first_cm[k]); tab.push_back((uint32_t)boxes[lo + k].t); }
  const size_t o_segs = tab.size();
  for (size_t k = 0; k < B; ++k) { tab.push_back((uint32_t)first[k]); tab.push_back((uint32_t)boxes[lo + k].n); }
  const size_t tab_bytes = ((tab.size() * 4 + 15) / 16) * 16;
  const bool dev = space != MPVSS_HOST;
  // pinned staging, 16-byte aligned parts: [tables | 5 B source pointers (device space)] [challenge per share] [host space: positions,
  // commitments, public keys, shares, responses] [back: X, a1, a2, flags; device space: shares, responses]
  auto al = [](size_t v) { return (v + 15) / 16 * 16; };
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += al(bytes); return at; };
  const size_t p_tab = take(tab_bytes + (dev ? 5 * B * sizeof(void*) : 0)), p_ch = take(S * 32);
  const size_t p_pos = take(dev ? 0 : S * 8), p_cm = take(dev ? 0 : T * L), p_y = take(dev ? 0 : S * L), p_Y = take(dev ? 0 : S * L),
               p_r = take(dev ? 0 : S * 32);
  const size_t p_X = take(S * L), p_a1 = take(S * L), p_a2 = take(S * L), p_ok = take(T + 2 * S);
  const size_t p_Yb = take(dev ? S * L : 0), p_rb = take(dev ? S * 32 : 0);
  spans_reset(ctx);
  RET_IF(ensure_pinned(ctx, off));
  uint8_t* pin = (uint8_t*)ctx->pin;
  StreamDrain drain{ctx};   // (the staging is the context's: nothing of this pass may be pending in it afterwards)
  memcpy(pin + p_tab, tab.data(), tab.size() * 4);
  const uint8_t** srcs = (const uint8_t**)(pin + p_tab + tab_bytes);      // [array][box]: positions, commitments, y, Y, r
  for (size_t k = 0; k < B; ++k) {
    const mpvss_ec_box& b = boxes[lo + k];
    for (size_t i = first[k]; i < first[k + 1]; ++i) memcpy(pin + p_ch + i * 32, b.challenge_host, 32);
    if (dev) {
      srcs[0 * B + k] = (const uint8_t*)b.positions;
      srcs[1 * B + k] = b.commitments;
      srcs[2 * B + k] = b.pubkeys;
      srcs[3 * B + k] = b.shares;
      srcs[4 * B + k] = b.responses;
    } else {
      memcpy(pin + p_pos + first[k] * 8, b.positions, b.n * 8);
      memcpy(pin + p_cm + first_cm[k] * L, b.commitments, b.t * L);
      memcpy(pin + p_y + first[k] * L, b.pubkeys, b.n * L);
      memcpy(pin + p_Y + first[k] * L, b.shares, b.n * L);
      memcpy(pin + p_r + first[k] * 32, b.responses, b.n * 32);
    }
  }
  const uint32_t* comb;
  RET_IF(ec_comb(ctx, group, &comb));
  const size_t okn = T + 2 * S;
  RET_IF(ensure(ctx, w.e, p_ch - p_tab));
  RET_IF(ensure(ctx, w.chal, std::max<size_t>(S * 32, 64)));
  RET_IF(ensure(ctx, w.pos, S * 8));
  RET_IF(ensure(ctx, w.cmenc, T * L));
  RET_IF(ensure(ctx, w.cm, T * pw * 4));
  RET_IF(ensure(ctx, w.a, S * L));
  RET_IF(ensure(ctx, w.b, S * L));
  RET_IF(ensure(ctx, w.d, S * 32));
  RET_IF(ensure(ctx, w.ok, okn > 4096 ? okn : 4096));
  RET_IF(ensure(ctx, w.x, S * L));
  RET_IF(ensure(ctx, w.pts, S * pw * 4));
  RET_IF(ensure(ctx, w.o1, S * L));
  RET_IF(ensure(ctx, w.o2, S * L));
  hipStream_t s = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(w.e.p, pin + p_tab, p_ch - p_tab, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(w.chal.p, pin + p_ch, S * 32, hipMemcpyHostToDevice, s));
  const uint32_t* d_tiles = (const uint32_t*)w.e.p;
  const uint32_t *d_btab = d_tiles + o_btab, *d_segs = d_tiles + o_segs;
  if (dev) {                // every box's arrays lie in device buffers of their own: one gather launch per array, no copy per box
    const uint8_t* const* d_srcs = (const uint8_t* const*)((const uint8_t*)w.e.p + tab_bytes);
    LAUNCHCHK(ctx, ec_launch_gather_segments(d_srcs + 0 * B, d_segs, (int)B, 8, (uint8_t*)w.pos.p, s));
    LAUNCHCHK(ctx, ec_launch_gather_segments(d_srcs + 1 * B, d_btab, (int)B, (uint32_t)L, (uint8_t*)w.cmenc.p, s));
    LAUNCHCHK(ctx, ec_launch_gather_segments(d_srcs + 2 * B, d_segs, (int)B, (uint32_t)L, (uint8_t*)w.a.p, s));
    LAUNCHCHK(ctx, ec_launch_gather_segments(d_srcs + 3 * B, d_segs, (int)B, (uint32_t)L, (uint8_t*)w.b.p, s));
    LAUNCHCHK(ctx, ec_launch_gather_segments(d_srcs + 4 * B, d_segs, (int)B, 32, (uint8_t*)w.d.p, s));
  } else {
    HIPCHK(ctx, hipMemcpyAsync(w.pos.p, pin + p_pos, S * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(w.cmenc.p, pin + p_cm, T * L, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(w.a.p, pin + p_y, S * L, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(w.b.p, pin + p_Y, S * L, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(w.d.p, pin + p_r, S * 32, hipMemcpyHostToDevice, s));
  }
  uint8_t* ok = (uint8_t*)w.ok.p;
  const uint8_t *dr = (const uint8_t*)w.d.p, *dc = (const uint8_t*)w.chal.p;
  uint8_t *dX = (uint8_t*)w.x.p, *d1 = (uint8_t*)w.o1.p, *d2 = (uint8_t*)w.o2.p;
  // the launches of ONE box over the concatenation: decode, X (encodings and internal points), a2 = r y + c Y, a1 = r G + c X with
  // X handed over as internal points (EcBase::pts, as the forward-difference path does: no second decode of X)
  LAUNCHCHK(ctx, ec_launch_decode(group, (const uint8_t*)w.cmenc.p, (int)T, (uint32_t*)w.cm.p, ok, s));
  TIMED_LAUNCH(ctx, 0, ec_launch_commit_eval_tiles(group, (const uint32_t*)w.cm.p, d_tiles, (int)ntiles, d_btab, (const int64_t*)w.pos.p,
                                                   dX, (uint32_t*)w.pts.p, s));
  EcBase by, bY, bg, bX;
  by.enc = (const uint8_t*)w.a.p; by.enc_stride = L;
  bY.enc = (const uint8_t*)w.b.p; bY.enc_stride = L;
  RET_IF(ec_dual(ctx, gi, by, dr, 32, &bY, dc, 32, S, w.tab1, w.tab2, w.p2, d2, ok + T, ok + T + S));
  bg.generator = true;
  bX.pts = (const uint32_t*)w.pts.p;
  RET_IF(ec_dual(ctx, gi, bg, dr, 32, &bX, dc, 32, S, w.tab3, w.tab3, w.p1, d1, nullptr, nullptr));
  HIPCHK(ctx, hipMemcpyAsync(pin + p_X, dX, S * L, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(pin + p_a1, d1, S * L, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(pin + p_a2, d2, S * L, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(pin + p_ok, ok, okn, hipMemcpyDeviceToHost, s));
  if (dev) {
    HIPCHK(ctx, hipMemcpyAsync(pin + p_Yb, w.b.p, S * L, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(pin + p_rb, w.d.p, S * 32, hipMemcpyDeviceToHost, s));
  }
  RET_IF(spans_collect(ctx));                                       // the pass's one synchronisation
  const uint8_t *hX = pin + p_X, *h1 = pin + p_a1, *h2 = pin + p_a2, *hok = pin + p_ok;
  const uint8_t *hY = pin + (dev ? p_Yb : p_Y), *hr = pin + (dev ? p_rb : p_r);
  // The boxes' transcripts are independent: every thread takes a contiguous range of boxes.  A box's flags are judged in the order
  // ec_verify_block_absorb_locked looks at them: responses, then commitments, public keys, shares; the first of each.
  struct Refusal { const char* what = nullptr; size_t i = 0; bool scalar = false; };
  std::vector<Refusal> refused(B);
  // automatic: one thread per 512 shares of the run; 1 .. 16, never sized by the machine
  const size_t nth = std::min<size_t>((size_t)many::many_threads(hash_threads, S, 512), B);
  hsc::parallel_indices((unsigned)nth, [&](unsigned part) {
    for (size_t k = B * part / nth; k < B * (part + 1) / nth; ++k) {
      const mpvss_ec_box& b = boxes[lo + k];
      const size_t s0 = first[k], n = b.n, c0 = first_cm[k], t = b.t;
      Refusal& r = refused[k];
      for (size_t i = 0; i < n && !r.what; ++i)
        if (!scalar_canonical(gi, hr + (s0 + i) * 32)) r = Refusal{"responses", i, true};
      for (size_t i = 0; i < t && !r.what; ++i)
        if (!hok[c0 + i]) r = Refusal{"commitments", i, false};
      for (size_t i = 0; i < n && !r.what; ++i)
        if (!hok[T + s0 + i]) r = Refusal{"public keys", i, false};
      for (size_t i = 0; i < n && !r.what; ++i)
        if (!hok[T + S + s0 + i]) r = Refusal{"encrypted shares", i, false};
      if (r.what) continue;
      mpvss::Sha256 tr;                                             // dleq.rs:87-99, share order = array order
      ec_frame_shares(tr, hX, hY, h1, h2, L, s0, s0 + n);
      (void)mpvss_ec_transcript_verdict(group, (const uint8_t*)&tr, b.challenge_host, &verdicts[lo + k],
                                        digests32 ? digests32 + 32 * (lo + k) : nullptr);
    }
  });
  size_t good = 0;
  for (size_t k = 0; k < B; ++k) {                                  // in box order: the message is that of the last box turned down
    const Refusal& r = refused[k];
    if (!r.what) ++good;
    else if (r.scalar) (void)ec_report_bad_scalar(ctx, r.what, r.i);
    else (void)ec_report_bad_element(ctx, r.what, r.i);
  }
  if (good) {
    ++ctx->ec_many_passes;
    ctx->ec_many_grouped_boxes += good;
  }
  return MPVSS_OK;
}

}  // namespace

extern "C" int mpvss_ec_verify_many(mpvss_ctx* ctx, int group, int space, const mpvss_ec_box* boxes, size_t count, int depth,
                                    int hash_threads, int* verdicts, uint8_t* digests32) {
  if (!ctx) return MPVSS_E_INVALID;
  if (count == 0) return MPVSS_OK;
  int mode;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ec_info(group)) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_verify_many: unknown group");
    if (!boxes || !verdicts) return fail(ctx, MPVSS_E_INVALID, "ec_verify_many: bad argument");
    mode = ctx->ec_box_groups;
  }
  const EcInfo* gi = ec_info(group);
  for (size_t i = 0; i < count; ++i) verdicts[i] = 0;
  if (digests32) memset(digests32, 0, 32 * count);       // a malformed box has no transcript: verdict 0, digest zero
  // X paths of up to MPVSS_EC_X_BATCH consecutive boxes of one shape in the same launches (0 / 1: every box on its own):
  // at a box not yet covered, the longest run of batchable boxes of its shape that starts there.  A batch workspace is
  // reused after `ring` batches: even with batches of two, more boxes than can be in flight lie in between.
  static const int xbatch = fd_env("MPVSS_EC_X_BATCH", 16);
  const size_t xB = xbatch > 1 ? (size_t)xbatch : 1;
  const size_t ring = mpvss_ctx::NSLOT / 2 + 2;
  std::vector<EcPre> pre(count);
  std::vector<char> has_pre(count, 0), looked(count, 0);
  size_t batch_no = 0;
  std::atomic<unsigned long long> finished{0};           // boxes the pipeline verified (turned-down and empty ones count nowhere)
  // the unchanged pipeline over the boxes [lo, hi): every box through a block slot of its own
  auto pipeline = [&](size_t lo, size_t hi) -> int {
    if (lo == hi) return MPVSS_OK;
    return run_box_pipeline(
        ctx, hi - lo, depth, hash_threads,
        [&](size_t rel, unsigned*) {
          const size_t b = lo + rel;
          const mpvss_ec_box& bx = boxes[b];
          if (xB > 1 && !looked[b]) {
            size_t B = 0;
            while (B < xB && b + B < hi && ec_x_box_batchable(space, boxes[b + B], bx.n, bx.t)) ++B;
            for (size_t i = 0; i < std::max<size_t>(B, 1); ++i) looked[b + i] = 1;
            if (B >= 2) {
              while (ctx->ec_xb.size() < ring) ctx->ec_xb.push_back(new mpvss_ctx::XBatch());
              const int rc = ec_x_batch_compute(ctx, gi, space, boxes + b, B, *ctx->ec_xb[batch_no++ % ring], &pre[b]);
              if (rc == MPVSS_OK) for (size_t i = 0; i < B; ++i) has_pre[b + i] = 1;
              else if (rc != 1) return rc;
            }
          }
          return ec_verify_block_compute_locked(ctx, group, space, bx.commitments, bx.t, bx.positions, bx.pubkeys, bx.shares,
                                                bx.responses, bx.n, bx.challenge_host, has_pre[b] ? &pre[b] : nullptr);
        },
        [&](size_t rel, const uint8_t* state) {
          const size_t idx = lo + rel;
          if (boxes[idx].n > 0) ++finished;
          return mpvss_ec_transcript_verdict(group, state, boxes[idx].challenge_host, &verdicts[idx],
                                             digests32 ? digests32 + 32 * idx : nullptr);
        });
  };
  // The runs of many::walk: small boxes (ec_box_small) travel together, (n, t) against MAX_CHUNK shares and MAX_CHUNK commitments.
  // A run of two or more boxes is one grouped pass; every other box -- a run of one, an empty, malformed or larger box -- stays
  // where it is and goes through the pipeline, which is applied to the stretches between the passes (the X-batch look-ahead
  // works inside a stretch).  Every box that is not small ends a run, so a run is the range [front, back].  `depth` means nothing
  // inside a pass.
  int rc = MPVSS_OK;
  size_t stretch = 0;                                    // first box not yet handed to the pipeline or to a pass
  if (mode == 1)
    rc = many::walk(
        count, MAX_CHUNK, MAX_CHUNK, [&](size_t i) { return ec_box_small(gi, boxes[i]) ? many::GROUPED : many::ALONE; },
        [&](size_t i) { return many::Cost{boxes[i].n, boxes[i].t}; }, [](size_t, size_t) { return true; },
        [](size_t) { return MPVSS_OK; },
        [&](const std::vector<size_t>& run) -> int {
          RET_IF(pipeline(stretch, run.front()));
          stretch = run.back() + 1;
          std::lock_guard<std::mutex> lk(ctx->mu);
          return ec_many_run(ctx, gi, space, boxes, run.front(), run.back() + 1, hash_threads, verdicts, digests32);
        });
  if (rc == MPVSS_OK) rc = pipeline(stretch, count);
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->ec_many_single_boxes += finished.load();
  return rc;
}

extern "C" int mpvss_ctx_set_ec_box_groups(mpvss_ctx* ctx, int mode) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode != 0 && mode != 1) return fail(ctx, MPVSS_E_INVALID, "set_ec_box_groups: mode must be 0 (every box on its own) or 1 (automatic)");
  ctx->ec_box_groups = mode;
  return MPVSS_OK;
}

extern "C" int mpvss_ec_verify_many_stats(mpvss_ctx* ctx, unsigned long long* passes, unsigned long long* grouped_boxes,
                                          unsigned long long* single_boxes) {
  return many_stats(ctx, &mpvss_ctx::ec_many_passes, &mpvss_ctx::ec_many_grouped_boxes, &mpvss_ctx::ec_many_single_boxes, passes,
                    grouped_boxes, single_boxes);
}

// ---- verify_share, batched (participant.rs:1346-1371, 1789-1814) ---------------------------------------------
// compute (enqueue only) / absorb (wait, validate, hand out the verdicts): several batches in flight, like the MODP form.
// Slot kind 3.  Staging: [6 n] flag / verdict bytes as the kernels leave them (decode flags of the four bases, scalar
// flags, verdicts), then -- host callers -- a pinned copy of the five input arrays.
namespace {
int ec_verify_shares_compute_locked(mpvss_ctx* ctx, int group, int space, const uint8_t* pk, const uint8_t* s,
                                    const uint8_t* y, const uint8_t* c, const uint8_t* r, size_t n,
                                    uint8_t* verdicts_dev_out) {
  const EcInfo* gi = ec_info(group);
  if (!gi) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_verify_shares: unknown group");
  if (n > 0 && (!pk || !s || !y || !c || !r || n > 0x7fffffff)) return fail(ctx, MPVSS_E_INVALID, "ec_verify_shares: bad argument");
  BlockEnqueue be(ctx, 3, n, "ec_verify_shares");
  RET_IF(be.rc);
  mpvss_ctx::BlockSlot& sl = be.sl;
  sl.group = group;
  if (n == 0) return be.commit_empty();
  const uint32_t* comb;
  RET_IF(ec_comb(ctx, group, &comb));          // built once, on the context's stream
  RET_IF(be.enter());
  EcWork& w = sl.ecw;
  const size_t L = gi->enc;
  RET_IF(be.pin(6 * n + (space == MPVSS_HOST ? 3 * n * L + 2 * n * 32 : 0)));
  uint8_t* hok = (uint8_t*)sl.pin;
  if (space == MPVSS_HOST) {
    uint8_t* in = hok + 6 * n;
    memcpy(in, pk, n * L); pk = in; in += n * L;
    memcpy(in, s, n * L); s = in; in += n * L;
    memcpy(in, y, n * L); y = in; in += n * L;
    memcpy(in, c, n * 32); c = in; in += n * 32;
    memcpy(in, r, n * 32); r = in;
  }
  const void *dpk, *ds, *dy, *dc, *dr;
  RET_IF(stage_in(ctx, space, pk, n * L, w.a, &dpk));
  RET_IF(stage_in(ctx, space, s, n * L, w.b, &ds));
  RET_IF(stage_in(ctx, space, y, n * L, w.c, &dy));
  RET_IF(stage_in(ctx, space, r, n * 32, w.d, &dr));
  RET_IF(stage_in(ctx, space, c, n * 32, w.e, &dc));
  RET_IF(ensure(ctx, w.o1, n * L));
  RET_IF(ensure(ctx, w.o2, n * L));
  const size_t okn = n > 4096 ? n : 4096;
  RET_IF(ensure(ctx, w.ok, 6 * okn));          // decode flags of the four bases, scalar flags, verdicts
  uint8_t *d1 = (uint8_t*)w.o1.p, *d2 = (uint8_t*)w.o2.p;
  uint8_t *ok = (uint8_t*)w.ok.p, *oksc = ok + 4 * n, *dv = ok + 5 * n;
  // a1 = r*G + c*pk ; a2 = r*S + c*Y     (dleq.rs:66-84 via participant.rs:1361-1370)
  EcBase bg, bpk, bs, by;
  bg.generator = true;
  bpk.enc = (const uint8_t*)dpk; bpk.enc_stride = L;
  bs.enc = (const uint8_t*)ds; bs.enc_stride = L;
  by.enc = (const uint8_t*)dy; by.enc_stride = L;
  RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dr, 32, &bpk, (const uint8_t*)dc, 32, n, w.tab1, w.tab2, w.p1, d1, ok, ok + n));
  RET_IF(ec_dual(ctx, gi, bs, (const uint8_t*)dr, 32, &by, (const uint8_t*)dc, 32, n, w.tab1, w.tab2, w.p2, d2, ok + 2 * n, ok + 3 * n));
  // K7: per-share SHA-256 / SHA-512 of the framed elements, hash_to_scalar, comparison with c_i -- on the device
  TIMED_LAUNCH(ctx, 0, verdict_launch_ec(group, (const uint8_t*)dpk, (const uint8_t*)dy, d1, d2, (const uint8_t*)dc,
                                         (const uint8_t*)dr, (int)n, dv, oksc, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(hok, ok, 6 * n, hipMemcpyDeviceToHost, ctx->stream));
  if (verdicts_dev_out) HIPCHK(ctx, hipMemcpyAsync(verdicts_dev_out, dv, n, hipMemcpyDeviceToDevice, ctx->stream));
  return be.commit();
}

int ec_verify_shares_absorb_locked(mpvss_ctx* ctx, std::unique_lock<std::mutex>& lk, uint8_t* verdicts_host,
                                   const unsigned long long* own_pos = nullptr) {
  mpvss_ctx::BlockSlot* slp = select_block(ctx, own_pos, own_pos != nullptr, 3, 3, "ec_verify_shares_absorb");
  if (!slp) return MPVSS_E_INVALID;
  mpvss_ctx::BlockSlot& sl = *slp;
  const size_t n = sl.n;
  const uint8_t* hok = (const uint8_t*)sl.pin;
  long bad_scalar = -1, bad_elem = -1;
  Absorbed a;
  RET_IF(absorb_block(ctx, lk, sl, a, [&](bool done) {
    if (!done) return;
    for (size_t i = 0; i < n && bad_scalar < 0; ++i)
      if (!hok[4 * n + i]) bad_scalar = (long)i;
    for (size_t i = 0; i < 4 * n && bad_elem < 0; ++i)
      if (!hok[i]) bad_elem = (long)(i % n);
    if (bad_scalar < 0 && bad_elem < 0 && verdicts_host) memcpy(verdicts_host, hok + 5 * n, n);
  }));
  if (!a.waited) return MPVSS_OK;
  if (a.e != hipSuccess) return fail(ctx, MPVSS_E_DEVICE, "ec_verify_shares_absorb: hipEventSynchronize", a.e);
  if (bad_scalar >= 0) return ec_report_bad_scalar(ctx, "ec_verify_shares: response or challenge", (size_t)bad_scalar);
  if (bad_elem >= 0) return ec_report_bad_element(ctx, "share boxes", (size_t)bad_elem);
  RET_IF(spans_sum(ctx, sl.spans, ctx->kernel_ms));
  return MPVSS_OK;
}
}  // namespace

extern "C" int mpvss_ec_verify_shares_compute(mpvss_ctx* ctx, int group, int space, const uint8_t* pk, const uint8_t* s,
                                              const uint8_t* y, const uint8_t* c, const uint8_t* r, size_t n,
                                              uint8_t* verdicts_dev_out) {
  if (!ctx) return MPVSS_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ec_verify_shares_compute_locked(ctx, group, space, pk, s, y, c, r, n, verdicts_dev_out);
}
extern "C" int mpvss_ec_verify_shares_absorb(mpvss_ctx* ctx, uint8_t* verdicts_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  return ec_verify_shares_absorb_locked(ctx, lk, verdicts_host);
}

extern "C" int mpvss_ec_verify_shares(mpvss_ctx* ctx, int group, int space, const uint8_t* pk, const uint8_t* s,
                                      const uint8_t* y, const uint8_t* c, const uint8_t* r, size_t n,
                                      uint8_t* verdicts_host) {
  if (!ctx) return MPVSS_E_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  if (!ec_info(group)) return fail(ctx, MPVSS_E_UNSUPPORTED, "ec_verify_shares: unknown group");
  if (n == 0) return MPVSS_OK;
  if (!pk || !s || !y || !c || !r || !verdicts_host || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "ec_verify_shares: bad argument");
  RET_IF(wait_for_room(ctx, lk));
  RET_IF(ec_verify_shares_compute_locked(ctx, group, space, pk, s, y, c, r, n, nullptr));
  const unsigned long long blk = ctx->own_last(1);
  return ec_verify_shares_absorb_locked(ctx, lk, verdicts_host, &blk);
}

// ---- distribute_secret, group part (participant.rs:1094-1274, 1573-1717) ------------------------------------
extern "C" int mpvss_ec_distribute(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                   const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values,
                                   const uint8_t* witnesses, size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out,
                                   uint8_t* a2_out, uint8_t* digest32_out) {
  EC_PROLOGUE("ec_distribute");
  if (n > 0 && (!commitments || !positions || !pubkeys || !p_values || !witnesses || !x_out || !y_out || !a1_out ||
                !a2_out || t == 0 || t > 0x7fffffff || n > 0x7fffffff))
    return fail(ctx, MPVSS_E_INVALID, "ec_distribute: bad argument");
  if (t > n) return fail(ctx, MPVSS_E_INVALID, "ec_distribute: threshold > number of public keys (participant.rs:1100)");
  mpvss::Sha256 transcript;
  if (n > 0) {
    RET_IF(ec_check_scalars(ctx, gi, space, p_values, n, "polynomial values"));
    RET_IF(ec_check_scalars(ctx, gi, space, witnesses, n, "witnesses"));
    RET_IF(ec_stage_commitments(ctx, gi, w, space, commitments, t));
    const int64_t *dpos, *hpos;
    RET_IF(ec_stage_positions(ctx, w, space, positions, n, &dpos, &hpos));
    const void *dy, *dp, *dw;
    RET_IF(stage_in(ctx, space, pubkeys, n * gi->enc, w.a, &dy));
    RET_IF(stage_in(ctx, space, p_values, n * 32, w.d, &dp));
    RET_IF(stage_in(ctx, space, witnesses, n * 32, w.e, &dw));
    uint8_t *dX = x_out, *dY = y_out, *d1 = a1_out, *d2 = a2_out;
    if (space == MPVSS_HOST) {
      RET_IF(ensure(ctx, w.x, n * gi->enc)); RET_IF(ensure(ctx, w.b, n * gi->enc));
      RET_IF(ensure(ctx, w.o1, n * gi->enc)); RET_IF(ensure(ctx, w.o2, n * gi->enc));
      dX = (uint8_t*)w.x.p; dY = (uint8_t*)w.b.p; d1 = (uint8_t*)w.o1.p; d2 = (uint8_t*)w.o2.p;
    }
    const size_t okn = n > 4096 ? n : 4096;
    RET_IF(ensure(ctx, w.ok, 2 * okn));
    uint8_t* ok = (uint8_t*)w.ok.p;
    const int* gate;
    const uint32_t* pts;
    RET_IF(ec_eval_x(ctx, gi, w, t, hpos, dpos, n, dX, &gate, &pts));
    EcBase by, bg;
    by.enc = (const uint8_t*)dy; by.enc_stride = gi->enc;
    bg.generator = true;
    // the table of y_i serves both Y = p * y (participant.rs:1190) and a2 = w * y (dleq.rs:214-216)
    RET_IF(ec_dual(ctx, gi, by, (const uint8_t*)dp, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p1, dY, ok, nullptr));
    RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dw, 32, nullptr, nullptr, 0, n, w.tab2, w.tab2, w.p1, d1, nullptr, nullptr));   // a1 = w * G
    by.table = (const uint32_t*)w.tab1.p;
    RET_IF(ec_dual(ctx, gi, by, (const uint8_t*)dw, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p2, d2, ok + n, nullptr));   // a2 = w * y
    RET_IF(ensure_pinned(ctx, n * gi->enc * 4));
    uint8_t* hX = (uint8_t*)ctx->pin;
    uint8_t* hY = hX + n * gi->enc;
    uint8_t* h1 = hY + n * gi->enc;
    uint8_t* h2 = h1 + n * gi->enc;
    HIPCHK(ctx, hipMemcpyAsync(hX, dX, n * gi->enc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hY, dY, n * gi->enc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h1, d1, n * gi->enc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(h2, d2, n * gi->enc, hipMemcpyDeviceToHost, ctx->stream));
    RET_IF(ec_check_ok(ctx, ok, 2 * n, "public keys"));
    ec_frame_shares(transcript, hX, hY, h1, h2, gi->enc, 0, n);
    if (space == MPVSS_HOST) {
      memcpy(x_out, hX, n * gi->enc); memcpy(y_out, hY, n * gi->enc);
      memcpy(a1_out, h1, n * gi->enc); memcpy(a2_out, h2, n * gi->enc);
    }
    RET_IF(spans_collect(ctx));
  }
  if (digest32_out) transcript.final(digest32_out);
  return MPVSS_OK;
}

extern "C" int mpvss_ec_hash_to_scalar(int group, const uint8_t* data, size_t len, uint8_t out32[32]) {
  const EcInfo* gi = ec_info(group);
  if (!gi || (!data && len) || !out32) return MPVSS_E_INVALID;
  // Group::hash_to_scalar hashes `data` itself (secp256k1.rs:121-131 SHA-256, ristretto255.rs:196-205 SHA-512)
  ec_hash_to_scalar_bytes(gi, data, len, out32);
  return MPVSS_OK;
}

// ---- extract_secret_share, batched, EC groups (participant.rs:1282-1338, 1725-1781) ---------------------------
extern "C" int mpvss_ec_extract_shares(mpvss_ctx* ctx, int group, int space, const uint8_t* pk, const uint8_t* y,
                                       const uint8_t* xinv, const uint8_t* wit, size_t n, uint8_t* s_out,
                                       uint8_t* c_out_host) {
  EC_PROLOGUE("ec_extract_shares");
  if (n == 0) return MPVSS_OK;
  if (!pk || !y || !xinv || !wit || !s_out || !c_out_host || n > 0x7fffffff)
    return fail(ctx, MPVSS_E_INVALID, "ec_extract_shares: bad argument");
  RET_IF(ec_check_scalars(ctx, gi, space, xinv, n, "inverse private keys"));
  RET_IF(ec_check_scalars(ctx, gi, space, wit, n, "witnesses"));
  const void *dy, *dxi, *dw;
  RET_IF(stage_in(ctx, space, y, n * gi->enc, w.a, &dy));
  RET_IF(stage_in(ctx, space, xinv, n * 32, w.d, &dxi));
  RET_IF(stage_in(ctx, space, wit, n * 32, w.e, &dw));
  uint8_t* dS = s_out;
  if (space == MPVSS_HOST) { RET_IF(ensure(ctx, w.x, n * gi->enc)); dS = (uint8_t*)w.x.p; }
  RET_IF(ensure(ctx, w.o1, n * gi->enc));
  RET_IF(ensure(ctx, w.o2, n * gi->enc));
  const size_t okn = n > 4096 ? n : 4096;
  RET_IF(ensure(ctx, w.ok, okn));
  uint8_t *d1 = (uint8_t*)w.o1.p, *d2 = (uint8_t*)w.o2.p, *ok = (uint8_t*)w.ok.p;
  EcBase by, bg, bS;
  by.enc = (const uint8_t*)dy; by.enc_stride = gi->enc;
  bg.generator = true;
  RET_IF(ec_dual(ctx, gi, by, (const uint8_t*)dxi, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p1, dS, ok, nullptr));      // S = (1/x) * Y
  RET_IF(ec_dual(ctx, gi, bg, (const uint8_t*)dw, 32, nullptr, nullptr, 0, n, w.tab2, w.tab2, w.p2, d1, nullptr, nullptr));  // a1 = w * G
  bS.pts = (const uint32_t*)w.p1.p;          // S in internal coordinates: no decoding of what was just encoded
  RET_IF(ec_dual(ctx, gi, bS, (const uint8_t*)dw, 32, nullptr, nullptr, 0, n, w.tab1, w.tab2, w.p2, d2, nullptr, nullptr));  // a2 = w * S
  RET_IF(ensure_pinned(ctx, n * gi->enc * 3));
  uint8_t* hS = (uint8_t*)ctx->pin;
  uint8_t* h1 = hS + n * gi->enc;
  uint8_t* h2 = h1 + n * gi->enc;
  HIPCHK(ctx, hipMemcpyAsync(hS, dS, n * gi->enc, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(h1, d1, n * gi->enc, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(h2, d2, n * gi->enc, hipMemcpyDeviceToHost, ctx->stream));
  RET_IF(ec_check_ok(ctx, ok, n, "encrypted shares"));
  std::vector<uint8_t> hpk, hy;
  RET_IF(small_vec_to_host(ctx, space, pk, n * gi->enc, hpk));
  RET_IF(small_vec_to_host(ctx, space, y, n * gi->enc, hy));
  for (size_t i = 0; i < n; ++i) {
    mpvss::Sha256 h;
    ec_frame_update(h, hpk.data() + i * gi->enc, gi->enc);
    ec_frame_update(h, hy.data() + i * gi->enc, gi->enc);
    ec_frame_update(h, h1 + i * gi->enc, gi->enc);
    ec_frame_update(h, h2 + i * gi->enc, gi->enc);
    uint8_t digest[32];
    h.final(digest);
    ec_hash_to_scalar(gi, digest, c_out_host + i * 32);
  }
  if (space == MPVSS_HOST) memcpy(s_out, hS, n * gi->enc);
  RET_IF(spans_collect(ctx));
  return MPVSS_OK;
}
