/* mpvss_hip.h -- C ABI of the MI355X-native batch group-exponentiation engine for mpvss-rs.
 *
 * This is the drop-in boundary for ONE hot path of the reference crate: the modexp inner
 * loops behind `distribute_secret`, `DLEQ::prove/verify` and `verify_distribution_shares`.
 * A Rust `impl Group for HipModpGroup` binds these symbols with
 * `extern "C"`; nothing here exposes C++, HIP or torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MPVSS_E_* code; nothing throws or
 *     aborts across the boundary; `mpvss_last_error(ctx)` gives a human-readable reason.
 *     (The reference returns `false`/`None` for structural problems and only panics on
 *     programmer errors such as threshold > n, src/participant.rs:166 -> MPVSS_E_INVALID.)
 *   - the caller owns every buffer; the library keeps no pointer after a call returns.
 *   - `space` says where the array arguments live: MPVSS_HOST (ordinary host memory) or
 *     MPVSS_DEVICE (HIP device memory of the context's GPU, e.g. a torch tensor's
 *     data_ptr()).  Scalar-like arguments documented as "host" are always host pointers.
 *   - MODP-2048 encoding: every element and scalar is a fixed 256-byte big-endian unsigned
 *     integer (zero padded).  The reference's minimal-length `element_to_bytes`
 *     (src/groups/modp.rs:150-152) only matters inside the Fiat-Shamir transcript, which
 *     the library frames itself (src/dleq.rs:58-61).  Elements need not be reduced: like
 *     `BigInt::modpow` the engine reduces them mod q (src/groups/modp.rs:154-156 does no
 *     validation).  Positions are the 1-based share indices (src/participant.rs:186).
 *   - a context may be used from several host threads (calls are serialised internally);
 *     `Group: Send + Sync` in the reference (src/group.rs:24).
 */
#ifndef MPVSS_HIP_H
#define MPVSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPVSS_OK 0
#define MPVSS_E_INVALID (-1)   /* bad argument (null pointer, n == 0 where forbidden, t > n, position < 0) */
#define MPVSS_E_DEVICE (-2)    /* HIP runtime error (see mpvss_last_error) */
#define MPVSS_E_NOMEM (-3)     /* workspace allocation failed */
#define MPVSS_E_UNSUPPORTED (-4)

#define MPVSS_HOST 0
#define MPVSS_DEVICE 1

#define MPVSS_MODP_BYTES 256   /* element / scalar width of the RFC 3526 group-14 encoding */

typedef struct mpvss_ctx mpvss_ctx;

/* ---- context ------------------------------------------------------------------------ */

/* Optional, process-wide, and only meaningful BEFORE the process's first HIP call (any library's): puts
 * GPU_MAX_HW_QUEUES=8 into the environment unless the variable is already set -- the block pipeline keeps one stream
 * pair per box in flight and wants 8 hardware queues (the runtime's default is 4; 16 or more oversubscribe the
 * hardware).  Returns 1 when it set the variable, 0 when a value was already there.  Not thread-safe against
 * concurrent getenv: call it at the top of main, or set the variable in the launcher instead.  The library never
 * changes the environment on its own. */
int mpvss_process_init(void);

/* Number of visible HIP devices (0 when there is no GPU; the library never falls back to
 * a CPU path -- every compute entry point then fails with MPVSS_E_DEVICE). */
int mpvss_device_count(void);

/* Create an engine bound to one GPU.  Replaces `ModpGroup::new()` (src/groups/modp.rs:44-69)
 * as the object the host-side Group impl holds in its `Arc`. */
int mpvss_ctx_create(int device_id, mpvss_ctx** out);
void mpvss_ctx_destroy(mpvss_ctx* ctx);
const char* mpvss_last_error(const mpvss_ctx* ctx);

/* Optional: run the engine's kernels on a caller-provided hipStream_t (passed as void*). */
int mpvss_ctx_set_stream(mpvss_ctx* ctx, void* hip_stream);
/* Block until everything queued by this context has finished. */
int mpvss_ctx_synchronize(mpvss_ctx* ctx);

/* ---- Group operations, batched ------------------------------------------------------- */

/* out[i] = bases[i]^exps[i] mod q.            Replaces n calls of ModpGroup::exp
 * (src/groups/modp.rs:122-128).  bases/exps/out: n x 256 bytes. */
int mpvss_modp_batch_exp(mpvss_ctx* ctx, int space, const uint8_t* bases, const uint8_t* exps, size_t n,
                         uint8_t* out);

/* out[i] = a[i]*b[i] mod q.                   Replaces ModpGroup::mul (src/groups/modp.rs:130-132). */
int mpvss_modp_batch_mul(mpvss_ctx* ctx, int space, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);

/* out[i] = base^exps[i] mod q for ONE base (host pointer, 256 bytes): the shape of
 * generate_public_key (modp.rs:176-178), commitments C_j = g^a_j (participant.rs:189-193) and
 * a1 = g^w (dleq.rs:207-216). */
int mpvss_modp_batch_exp_fixed_base(mpvss_ctx* ctx, int space, const uint8_t* base_host, const uint8_t* exps,
                                    size_t n, uint8_t* out);

/* ---- the commitment multi-exp -------------------------------------------------------- */

/* X[i] = prod_{j<t} C_j^(positions[i]^j mod (q-1)) mod q.
 * Replaces the loop at src/participant.rs:423-434 (= 207-215, = src/mpvss.rs:110-123).
 * commitments: t x 256 bytes; positions: n int64 (each >= 0); x_out: n x 256 bytes. */
int mpvss_modp_commit_eval(mpvss_ctx* ctx, int space, const uint8_t* commitments, size_t t,
                           const int64_t* positions, size_t n, uint8_t* x_out);

/* ---- DLEQ verifier commitments -------------------------------------------------------- */

/* a1[i] = g1^r[i] * h1[i]^c_i,  a2[i] = g2[i]^r[i] * h2[i]^c_i   (src/dleq.rs:66-84).
 * g1_host: one shared 256-byte base (host pointer).  c: one shared 256-byte challenge when
 * c_per_share == 0 (always a host pointer), else n x 256 bytes in `space`.
 * h1, g2, h2, r, a1_out, a2_out: n x 256 bytes in `space`. */
int mpvss_modp_dleq_commitments(mpvss_ctx* ctx, int space, const uint8_t* g1_host, const uint8_t* h1,
                                const uint8_t* g2, const uint8_t* h2, const uint8_t* r, const uint8_t* c,
                                int c_per_share, size_t n, uint8_t* a1_out, uint8_t* a2_out);

/* ---- verify_distribution_shares ------------------------------------------------------- */

/* Whole-box verification, src/participant.rs:399-455 (= src/mpvss.rs:90-144):
 *   for each share i (in array order): X_i (commit_eval), (a1_i, a2_i) = DLEQ commitments with
 *   (g, X_i, y_i, Y_i, r_i, c); transcript += framed(X_i) framed(Y_i) framed(a1_i) framed(a2_i)
 *   (minimal-length big-endian bytes, u64-BE length prefix, src/dleq.rs:58-61,87-99);
 *   *verdict = ( int(SHA256(SHA256(transcript))) mod (q-1)/2 == challenge ).
 * commitments t x 256; positions n; pubkeys (y_i), shares (Y_i), responses (r_i): n x 256, all in
 * `space`.  challenge: 256 bytes, host.  Outputs are host pointers: verdict (0/1),
 * digest32_out (optional, SHA-256 of the transcript), and optional n x 256 dumps of X, a1, a2
 * (pass NULL to skip).  An empty box (n == 0) hashes the empty transcript, as the reference does. */
int mpvss_modp_verify_distribution(mpvss_ctx* ctx, int space, const uint8_t* commitments, size_t t,
                                   const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                   const uint8_t* responses, size_t n, const uint8_t* challenge_host,
                                   int* verdict, uint8_t* digest32_out, uint8_t* x_out_host,
                                   uint8_t* a1_out_host, uint8_t* a2_out_host);

/* Sharded form of the same verification (one engine per GPU, contiguous blocks of shares per
 * engine, blocks absorbed in share order).  `state` is an opaque MPVSS_TRANSCRIPT_STATE_BYTES
 * running-hash state that travels from the engine holding block k to the one holding block k+1:
 *   mpvss_transcript_init(state);
 *   for each block in order:  ..._verify_block_compute(block);  ..._verify_block_absorb(state);
 *   mpvss_modp_transcript_verdict(state, challenge, &verdict, digest);
 * `compute` only enqueues GPU work (kernels + device-to-host copies) and returns; `absorb` waits
 * for it, so the wait for the previous block's state overlaps this block's GPU work.
 * Up to MPVSS_BLOCK_SLOTS blocks may be in flight per engine (compute, compute, ..., absorb, absorb in FIFO order): the
 * host hash of box k then overlaps the GPU work of boxes k+1.. (bench.py).
 * mpvss_modp_verify_distribution == init + compute + absorb + verdict on one engine. */
#define MPVSS_TRANSCRIPT_STATE_BYTES 128
/* blocks of the block API that may be in flight in one context (any mix of the compute calls below) */
#define MPVSS_BLOCK_SLOTS 64
void mpvss_transcript_init(uint8_t* state);
int mpvss_modp_verify_block_compute(mpvss_ctx* ctx, int space, const uint8_t* commitments, size_t t,
                                    const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                    const uint8_t* responses, size_t n, const uint8_t* challenge_host);
int mpvss_modp_verify_block_absorb(mpvss_ctx* ctx, uint8_t* state, uint8_t* x_out_host, uint8_t* a1_out_host,
                                   uint8_t* a2_out_host);
/* mpvss_modp_verify_block_compute that also leaves one well-formedness byte per share in DEVICE memory
 * (wellformed_dev_out, n bytes, valid once the block has been absorbed): 1 iff 0 < y_i < q, 0 < Y_i < q and
 * r_i < q - 1, i.e. the three inputs of the share are canonical encodings.  The reference validates nothing here
 * (src/groups/modp.rs:154-156; src/participant.rs:408-448 hashes whatever comes out), so these bytes never enter the box
 * verdict: they are the per-share record that the ranks of a sharded verification all-gather over RCCL,
 * telling every rank which block holds a non-canonical share. */
int mpvss_modp_verify_block_compute_flags(mpvss_ctx* ctx, int space, const uint8_t* commitments, size_t t,
                                          const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                          const uint8_t* responses, size_t n, const uint8_t* challenge_host,
                                          uint8_t* wellformed_dev_out);
/* The same in two steps, for callers whose transcript state arrives from elsewhere (one rank of a sharded verification:
 * the state of box b comes from the previous rank): mpvss_block_claim takes the oldest block in flight (a verifier's or
 * dealer's distribution block of any of the three groups) and returns its ticket -- tickets count the blocks of this context in enqueue order --,
 * mpvss_modp_verify_block_absorb_claimed waits for and hashes exactly that block.  Several threads may hold claimed
 * blocks at once; every claimed block must be absorbed. */
int mpvss_block_claim(mpvss_ctx* ctx, unsigned long long* ticket_out);
int mpvss_modp_verify_block_absorb_claimed(mpvss_ctx* ctx, unsigned long long ticket, uint8_t* state,
                                           uint8_t* x_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host);
/* Host-only: extend the transcript with `count` 256-byte elements, each framed as
 * u64-BE(minimal length) || minimal-length big-endian bytes (src/dleq.rs:58-61, modp.rs:150-152). */
int mpvss_modp_transcript_absorb(uint8_t* state, const uint8_t* elements, size_t count);
int mpvss_modp_transcript_verdict(const uint8_t* state, const uint8_t* challenge_host, int* verdict,
                                  uint8_t* digest32_out);

/* Many boxes at once -- the situation of a participant that checks every dealer's box (each call of
 * src/participant.rs:399-455 is independent of the others).  The library pipelines them itself: the calling thread
 * enqueues the GPU work of up to `depth` boxes (1..16) ahead while `hash_threads` (1..8) library threads wait for the
 * boxes in order and hash their transcripts.  verdicts[i] / digests32[32 i .. 32 i + 31] (optional) belong to
 * boxes[i]; all array pointers of a box live in `space`, the challenge is a host pointer; `keyset` may be NULL
 * (registered keys: then `pubkeys` may be NULL, see below).  Equivalent to count calls of
 * mpvss_modp_verify_distribution. */
typedef struct mpvss_keyset mpvss_keyset;
typedef struct mpvss_modp_box {
  const uint8_t* commitments; size_t t;
  const int64_t* positions;
  const uint8_t* pubkeys; const uint8_t* shares; const uint8_t* responses; size_t n;
  const uint8_t* challenge_host;
  const mpvss_keyset* keyset; size_t key_offset;
} mpvss_modp_box;
int mpvss_modp_verify_many(mpvss_ctx* ctx, int space, const mpvss_modp_box* boxes, size_t count, int depth,
                           int hash_threads, int* verdicts, uint8_t* digests32);

/* The same pipeline for ONE box held by SEVERAL engines (one per GPU, src/participant.rs:399-455 with the participants
 * sharded): this engine verifies its contiguous block of every box; a box's transcript is one ordered hash, so the 128-byte
 * running state travels engine to engine through two callbacks the library calls on its own threads, several boxes at a time,
 * each box exactly once:
 *   state_in(user, box, state, 1)   fill in the state this engine's block of `box` starts from (may block until the engine before
 *                                   has sent it); return non-zero when an earlier engine failed on the box.  NULL: first engine.
 *   state_out(user, box, state, ok) hand the state on after the block has been absorbed (ok = 0: this or an earlier engine failed
 *                                   on the box, the state is zero).  NULL: last engine.
 * verdicts / digests32 come from this engine's final state: meaningful on the last engine.  wellformed_dev_out: NULL or `count`
 * device buffers of n bytes each that receive the shares' well-formedness flags (mpvss_modp_verify_block_compute_flags). */
typedef int (*mpvss_chain_cb)(void* user, size_t box, uint8_t* state, int ok);
int mpvss_modp_verify_many_chained(mpvss_ctx* ctx, int space, const mpvss_modp_box* boxes, size_t count, int depth,
                                   int hash_threads, uint8_t* const* wellformed_dev_out, mpvss_chain_cb state_in,
                                   mpvss_chain_cb state_out, void* user, int* verdicts, uint8_t* digests32);

/* ---- registered public keys (opt-in) ---------------------------------------------------- */

/* In a PVSS deployment the participants' public keys are long-lived: every dealer distributes to the same keys, so
 * a verifier checks many boxes against one key set (src/participant.rs:399-455 takes the same `publickeys` each
 * time).  A key set holds, in HBM, per-key tables for y_i^r (295 KB per key: 19.3 GB for 65536 keys) built once
 * (about as much work as verifying 1.5 boxes); verify_block_compute_keyset then computes a2_i = y_i^r_i * Y_i^c with
 * 613 products instead of 2 620.  Results are identical to mpvss_modp_verify_block_compute on the same keys.
 * Shares i of the call use keys key_offset + i of the set.  Destroy a key set only after the blocks using it have
 * been absorbed.  The DEALER to registered keys (round 6: mpvss_modp_deal_compute_keyset, and mpvss_modp_deal / mpvss_modp_distribute
 * through the cross-call cache below) takes Y_i = y_i^P(i) and a2_i = y_i^w_i (participant.rs:219, dleq.rs:213-216) from the same
 * tables: 2 x 548 instead of 2 865 Montgomery operations per share, byte-identical results. */
int mpvss_modp_keyset_create(mpvss_ctx* ctx, int space, const uint8_t* pubkeys, size_t n, mpvss_keyset** out);
/* The same behind the UNCHANGED call (round 5): with min_boxes >= 2, mpvss_modp_verify_many builds the tables by itself for every
 * public-key array that at least min_boxes large boxes (more shares than the grouped small boxes have) of ONE call present -- the
 * same pointer and n inside one call is the same array: exact, nothing is hashed or compared -- uses them for those boxes and frees
 * them when the call returns.  Building costs about one box of GPU time (60 ms per 65536 keys, 295 KB of HBM per key); a box then
 * takes 37 instead of 59 ms: it pays from the third box.  What a verifier of many dealers' boxes against the same participants
 * (src/participant.rs:399-455 with the same `publickeys` each time) gets without touching its code.  0 (the default): off.
 * While either key cache is on the context keeps the table BUFFER of the last set it dropped (one buffer) for the next set it builds
 * -- allocating 19 GB can cost ten times what building the tables does --; it is released when both caches are off, with the
 * context, or as soon as a workspace allocation of the context fails for lack of memory.
 * Returns the previous setting, or a negative error. */
int mpvss_ctx_set_key_cache(mpvss_ctx* ctx, int min_boxes);
/* Call tables (ON by default, threshold 3): when at least `min_boxes` large boxes of one mpvss_modp_verify_many /
 * mpvss_modp_verify_many_chained call present the same DEVICE-resident key array (same pointer, same n; boxes without a key set,
 * 16 384 < n <= one chunk, challenge of at most 256 bits), the library builds eight rows of 32 powers per key once for the call
 * (72 KB per key, 4.8 GB for 65 536 keys; on a low-priority stream, beside the first boxes' X paths) and those boxes' a2 = y^r Y^c
 * takes them: 255 of the 2 046 squarings under y^r, no window table of y per box.  Same bytes, verdicts and digests.  The buffer stays
 * with the context between calls; it is freed when the feature is switched off, when a workspace allocation runs out of memory and
 * with the context.  Any failure costs speed, not the call.  min_boxes: 0 switches the feature off, >= 2 sets the threshold;
 * returns the previous value (negative: error).  MPVSS_CALL_TABLES=0 in the environment: off for every context of the process.
 * A box the key cache above takes goes through the key cache. */
int mpvss_ctx_set_call_tables(mpvss_ctx* ctx, int min_boxes);
/* builds: calls that built rows; boxes_served: boxes whose a2 took them (either pointer may be null) */
int mpvss_call_tables_stats(mpvss_ctx* ctx, unsigned long long* builds_out, unsigned long long* boxes_served_out);
/* ... and ACROSS calls, for callers that verify ONE box per call (the crate's call shape, src/participant.rs:399-455) against the
 * same participants again and again (round 6): with max_sets >= 1, mpvss_modp_verify_distribution identifies a HOST public-key array
 * by a SHA-256 tree hash of its bytes (16.8 MB per 65536 keys: eight slices hashed side by side, 1-2 ms, outside the context lock -- a
 * pointer may be re-used for other keys between calls, content may not), and the min_sightings-th box against the same array (default 2) builds its per-key
 * tables once; every later box against it takes the registered-key path.  At most max_sets (<= 8) sets have tables at a time (19.3 GB
 * per 65536 keys): the least recently used set that no block in flight reads makes room; tables that do not fit beside the block
 * slots' workspaces, or whose build fails, cost speed, not the call.  Same verdicts and digests as without the cache
 * (tests/test_gpu_keyset.py).  Boxes in device memory, small boxes (n <= 16384), boxes larger than one chunk and boxes whose challenge
 * does not fit 256 bits are left alone.  Dealers count as well: mpvss_modp_deal and mpvss_modp_distribute (host buffers, n > 16384)
 * look their key array up the same way, and a dealer's call is a sighting like a verifier's.  0: off (the default; frees the sets no
 * block reads).  Returns the previous max_sets, or a negative error. */
int mpvss_ctx_set_key_cache_lru(mpvss_ctx* ctx, int max_sets, int min_sightings);
void mpvss_modp_keyset_destroy(mpvss_ctx* ctx, mpvss_keyset* keyset);
size_t mpvss_modp_keyset_bytes(const mpvss_keyset* keyset);
int mpvss_modp_verify_block_compute_keyset(mpvss_ctx* ctx, int space, const uint8_t* commitments, size_t t,
                                           const int64_t* positions, const mpvss_keyset* keyset, size_t key_offset,
                                           const uint8_t* shares, const uint8_t* responses, size_t n,
                                           const uint8_t* challenge_host);

/* ---- verify_share, batched -------------------------------------------------------------- */

/* n independent share-box proofs, src/participant.rs:361-386 -> src/dleq.rs:275-302:
 *   a1 = G^r_i * pk_i^c_i, a2 = S_i^r_i * Y_i^c_i,
 *   verdicts[i] = ( hash_to_scalar(SHA256(framed(pk_i) framed(Y_i) framed(a1) framed(a2))) == c_i ).
 * Everything runs on the device, the hashing too (one lane per share, verdict_kernels.hip); only the n verdict bytes
 * come back.  pk, s (decrypted shares S_i), y (encrypted shares Y_i), c, r: n x 256 in `space`; verdicts: n bytes, host. */
int mpvss_modp_verify_shares(mpvss_ctx* ctx, int space, const uint8_t* pk, const uint8_t* s, const uint8_t* y,
                             const uint8_t* c, const uint8_t* r, size_t n, uint8_t* verdicts_host);
/* The same in two steps, so that several batches are in flight (they share the MPVSS_BLOCK_SLOTS block slots and the FIFO order
 * of mpvss_modp_verify_block_compute / _absorb): `compute` only enqueues GPU work and returns; `absorb` waits for the
 * oldest batch and hands out its verdict bytes.  verdicts_dev_out (optional, device memory, n bytes) receives the
 * verdicts in stream order as well -- the tensor a multi-GPU caller all-gathers over RCCL without a host round trip
 * (valid once the batch has been absorbed or mpvss_ctx_synchronize has returned). */
int mpvss_modp_verify_shares_compute(mpvss_ctx* ctx, int space, const uint8_t* pk, const uint8_t* s, const uint8_t* y,
                                     const uint8_t* c, const uint8_t* r, size_t n, uint8_t* verdicts_dev_out);
int mpvss_modp_verify_shares_absorb(mpvss_ctx* ctx, uint8_t* verdicts_host);

/* ---- distribute_secret, group part ------------------------------------------------------ */

/* Dealer side of src/participant.rs:160-286 with the randomness as INPUT (the reference draws
 * it from thread_rng, polynomial.rs:34-47 / modp.rs:162-174): given the polynomial values
 * p_i = P(i) mod (q-1) and witnesses w_i, computes
 *   X_i = prod C_j^(i^j)  (same loop as the verifier, participant.rs:207-215),
 *   Y_i = y_i^p_i (participant.rs:219), a1_i = g^w_i, a2_i = y_i^w_i (dleq.rs:207-216),
 * and the transcript digest SHA256(framed(X_i) framed(Y_i) framed(a1_i) framed(a2_i) ...)
 * (participant.rs:238-252).  Scalar-field work (responses r_i = w_i - p_i*c, polynomial
 * evaluation) stays on the host.  All arrays in `space`; digest32_out is a host pointer. */
int mpvss_modp_distribute(mpvss_ctx* ctx, int space, const uint8_t* commitments, size_t t,
                          const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values,
                          const uint8_t* witnesses, size_t n, uint8_t* x_out, uint8_t* y_out,
                          uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out);

/* The same in the compute / absorb form of the verifier's blocks (shared slots and FIFO order): `compute` enqueues the
 * GPU work of one block of shares and returns, `absorb` waits for it and extends the dealer's transcript `state` with
 * framed(X_i) framed(Y_i) framed(a1_i) framed(a2_i) in share order (participant.rs:238-245); the digest of the finished
 * transcript is mpvss_modp_transcript_verdict's digest32_out.  With space == MPVSS_DEVICE the four *_dev_out arrays (optional)
 * receive the results in HBM; absorb's host pointers are optional copies.
 * commitments == NULL: X_i is computed as g^p_i through the fixed-base comb -- the same element as the loop of
 * participant.rs:207-215 whenever the box's commitments are C_j = g^a_j of the polynomial behind p_i = P(i), which is what
 * the dealer of participant.rs:160-286 builds (t and positions are then unused). */
int mpvss_modp_distribute_compute(mpvss_ctx* ctx, int space, const uint8_t* commitments, size_t t, const int64_t* positions,
                                  const uint8_t* pubkeys, const uint8_t* p_values, const uint8_t* witnesses, size_t n,
                                  uint8_t* x_dev_out, uint8_t* y_dev_out, uint8_t* a1_dev_out, uint8_t* a2_dev_out);
int mpvss_modp_distribute_absorb(mpvss_ctx* ctx, uint8_t* state, uint8_t* x_out_host, uint8_t* y_out_host,
                                 uint8_t* a1_out_host, uint8_t* a2_out_host);
/* The dealer's block with the polynomial evaluation on the device as well (participant.rs:196-249 for one box or one block of
 * it): `compute` takes the t coefficients (host memory; 256-byte big-endian scalars) and n positions, public keys and witnesses
 * in HBM, evaluates p_i = P(position_i) mod (q-1) into p_dev_out (n x 256 bytes in HBM, kept for
 * mpvss_modp_dleq_responses_device) on the block's own stream and goes on as mpvss_modp_distribute_compute with
 * commitments == NULL: X_i = g^p_i, Y_i = y_i^p_i, a1_i = g^w_i, a2_i = y_i^w_i.  Absorbed by mpvss_modp_distribute_absorb (a
 * negative position fails the block there).  n <= 262144 shares per call. */
/* ... and the whole of it in one call for HOST buffers: P(i), X_i, Y_i, a1_i, a2_i, the transcript digest, the challenge
 * c = hash_to_scalar(digest) (participant.rs:251-252) and the responses r_i = w_i - P(i) c (:255-264), the 2048-bit scalar
 * arithmetic on the device too.  What is left to the caller of participant.rs:160-286 is drawing the polynomial and the
 * witnesses, the commitments C_j = g^a_j (mpvss_modp_batch_exp_fixed_base) and U.  x_out, a1_out, a2_out, digest32_out and
 * challenge_out256 are optional; t <= n < 2^31: like the reference, the call has no size limit of its own -- a box of more than
 * 262144 shares is cut into blocks internally (one transcript; the GPU works on one block while the host hashes the one before).
 * The call keeps its inputs and intermediate secrets in buffers of its own (a set per deal in flight from the context's pool:
 * several host threads may deal on one context at once), and zeroes P(i), the witnesses and the staged coefficients (device and
 * pinned host copies) before it returns. */
int mpvss_modp_deal(mpvss_ctx* ctx, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                    const uint8_t* pubkeys_host, const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out,
                    uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out256, uint8_t* r_out);
int mpvss_modp_deal_compute(mpvss_ctx* ctx, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                            const uint8_t* pubkeys_dev, const uint8_t* witnesses_dev, size_t n, uint8_t* p_dev_out,
                            uint8_t* x_dev_out, uint8_t* y_dev_out, uint8_t* a1_dev_out, uint8_t* a2_dev_out);
/* mpvss_modp_deal_compute to REGISTERED keys: shares i of the block go to keys key_offset + i of `keyset` (mpvss_modp_keyset_create);
 * Y_i and a2_i come from the key tables.  Same outputs as mpvss_modp_deal_compute with those keys. */
int mpvss_modp_deal_compute_keyset(mpvss_ctx* ctx, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                                   const mpvss_keyset* keyset, size_t key_offset, const uint8_t* witnesses_dev, size_t n,
                                   uint8_t* p_dev_out, uint8_t* x_dev_out, uint8_t* y_dev_out, uint8_t* a1_dev_out,
                                   uint8_t* a2_dev_out);

/* ---- elliptic-curve groups --------------------------------------------------------------------
 * The same entry points for the reference's two curve groups, selected by `group`:
 *   MPVSS_GROUP_SECP256K1    src/groups/secp256k1.rs:38-189     elements 33-byte SEC1 compressed
 *                            (the identity is 33 zero bytes, k256's GroupEncoding), scalars 32-byte big-endian
 *   MPVSS_GROUP_RISTRETTO255 src/groups/ristretto255.rs:45-253  elements 32-byte canonical ristretto255,
 *                            scalars 32-byte little-endian
 * Group law is written additively in the reference (exp = scalar multiplication, mul = point addition).
 * The reference's typed elements/scalars cannot hold an invalid encoding or a scalar >= the group
 * order; here such input makes the call fail with MPVSS_E_INVALID (mpvss_last_error names the index).
 * hash_to_scalar: SHA-256 then mod n (secp256k1.rs:121-131); SHA-512, little-endian, mod l
 * (ristretto255.rs:196-205).  Array shapes mirror the MODP calls with 256 replaced by the group's
 * element / scalar width; the challenge is 32 bytes. */
#define MPVSS_GROUP_SECP256K1 1
#define MPVSS_GROUP_RISTRETTO255 2

/* out[i] = scalars[i] * bases[i]      Secp256k1Group::exp secp256k1.rs:91-100, Ristretto255Group::exp ristretto255.rs:161-170 */
int mpvss_ec_batch_exp(mpvss_ctx* ctx, int group, int space, const uint8_t* bases, const uint8_t* scalars, size_t n,
                       uint8_t* out);
/* out[i] = a[i] + b[i]                ::mul secp256k1.rs:102-107, ristretto255.rs:172-177 */
int mpvss_ec_batch_mul(mpvss_ctx* ctx, int group, int space, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);
/* X[i] = sum_j (positions[i]^j mod order) * C_j     src/participant.rs:1404-1417 (secp256k1), 1847-1860 (ristretto255) */
int mpvss_ec_commit_eval(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                         const int64_t* positions, size_t n, uint8_t* x_out);
/* a1[i] = r[i]*g1 + c_i*h1[i], a2[i] = r[i]*g2[i] + c_i*h2[i]      src/dleq.rs:66-84 */
int mpvss_ec_dleq_commitments(mpvss_ctx* ctx, int group, int space, const uint8_t* g1_host, const uint8_t* h1,
                              const uint8_t* g2, const uint8_t* h2, const uint8_t* r, const uint8_t* c, int c_per_share,
                              size_t n, uint8_t* a1_out, uint8_t* a2_out);
/* out[i] = scalars[i] * G for the group's generator: keygen (secp256k1.rs:168-171, ristretto255.rs:239-242), commitments
 * C_j = a_j G (participant.rs:1145-1152, 1626-1633), a1 = w G (dleq.rs:207-211) -- fixed-base comb, no doublings */
int mpvss_ec_batch_exp_generator(mpvss_ctx* ctx, int group, int space, const uint8_t* scalars, size_t n, uint8_t* out);
/* src/participant.rs:1384-1442 (secp256k1), 1827-1885 (ristretto255).  Positions become scalars by
 * `Scalar::from(position as u64)` (participant.rs:1419, 1862), so a negative position wraps instead of failing. */
int mpvss_ec_verify_distribution(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                 const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                 const uint8_t* responses, size_t n, const uint8_t* challenge_host, int* verdict,
                                 uint8_t* digest32_out, uint8_t* x_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host);
/* The same split into compute (enqueue only) / absorb (wait, validate, hash) / verdict, sharing the MPVSS_BLOCK_SLOTS block slots
 * and the FIFO order of the MODP block calls, so that several boxes are in flight inside one context; and the
 * library-pipelined form for many boxes (see mpvss_modp_verify_many).  An invalid encoding or a response that is not
 * below the group order is reported by `absorb` (MPVSS_E_INVALID). */
int mpvss_ec_verify_block_compute(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                  const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                  const uint8_t* responses, size_t n, const uint8_t* challenge_host);
int mpvss_ec_verify_block_absorb(mpvss_ctx* ctx, uint8_t* state, uint8_t* x_out_host, uint8_t* a1_out_host,
                                 uint8_t* a2_out_host);
int mpvss_ec_transcript_absorb(int group, uint8_t* state, const uint8_t* elements, size_t count);
int mpvss_ec_transcript_verdict(int group, const uint8_t* state, const uint8_t* challenge_host, int* verdict,
                                uint8_t* digest32_out);
typedef struct mpvss_ec_box {
  const uint8_t* commitments; size_t t;
  const int64_t* positions;
  const uint8_t* pubkeys; const uint8_t* shares; const uint8_t* responses; size_t n;
  const uint8_t* challenge_host;
} mpvss_ec_box;
/* Many boxes of a curve group in one call: for every box, verdicts[i] and digests32[32 i ..] (may be NULL) are what
 * mpvss_ec_verify_distribution gives for that box.
 * RUNS OF SMALL BOXES (mode 1 of mpvss_ctx_set_ec_box_groups, the default): a box is small when 1 <= n < 4096, 1 <= t < 4096 (the
 * bound below which the forward differences never apply), all its pointers are set and its challenge is below the group order.  A
 * run is a maximal stretch of consecutive small boxes that hold at most MPVSS_MAX_CHUNK shares and at most MPVSS_MAX_CHUNK
 * commitments together.  A run of two or more boxes travels through the GPU as ONE dense batch -- one workgroup per 64 shares of
 * a box -- synchronously and with the context lock held for the pass (a few milliseconds); its transcripts are hashed by up to
 * hash_threads host threads (clamped to 1..16; <= 0: one per 512 shares of the run, at most 16, never by the machine's CPU count).
 * Every other box -- a run of one, an empty box, a malformed box, a box of n or t >= 4096 -- goes through a block slot of its own,
 * pipelined over the stretches between the runs: up to `depth` boxes enqueued ahead, hashed by hash_threads library threads (see
 * mpvss_modp_verify_many).  `depth` means nothing inside a run.
 * A box the engine turns down costs only itself, in a run or outside: verdict 0, a digest of zeros, and the call goes on and
 * returns MPVSS_OK.  That is an invalid encoding among commitments, public keys or shares, a response or challenge that is not
 * below the group order, a NULL pointer, t == 0 with n > 0.  mpvss_last_error names the reason and the index inside the box; of
 * the boxes of one run the last in box order.  A HIP error or a failed allocation ends the call.
 * mpvss_ctx_set_ec_box_groups: 0 = every box through a block slot of its own, 1 = automatic (the rule above); anything else is
 * MPVSS_E_INVALID.
 * mpvss_ec_verify_many_stats: since the context was created, both curves together: the grouped passes, the boxes they verified
 * and the boxes verified through a slot of their own.  Empty boxes and boxes turned down are in none of the counts.  Any pointer
 * may be NULL; no context is MPVSS_E_INVALID. */
int mpvss_ec_verify_many(mpvss_ctx* ctx, int group, int space, const mpvss_ec_box* boxes, size_t count, int depth,
                         int hash_threads, int* verdicts, uint8_t* digests32);
int mpvss_ctx_set_ec_box_groups(mpvss_ctx* ctx, int mode);
int mpvss_ec_verify_many_stats(mpvss_ctx* ctx, unsigned long long* passes, unsigned long long* grouped_boxes,
                               unsigned long long* single_boxes);
/* src/participant.rs:1346-1371 (secp256k1), 1789-1814 (ristretto255) */
int mpvss_ec_verify_shares(mpvss_ctx* ctx, int group, int space, const uint8_t* pk, const uint8_t* s, const uint8_t* y,
                           const uint8_t* c, const uint8_t* r, size_t n, uint8_t* verdicts_host);
/* The same in two steps (several batches in flight; they share the block slots and the FIFO order with the other block
 * calls): compute enqueues, absorb waits, validates (an invalid encoding or scalar is reported here) and hands out the
 * verdict bytes.  verdicts_dev_out: optional device buffer that receives the n verdict bytes in stream order. */
int mpvss_ec_verify_shares_compute(mpvss_ctx* ctx, int group, int space, const uint8_t* pk, const uint8_t* s,
                                   const uint8_t* y, const uint8_t* c, const uint8_t* r, size_t n,
                                   uint8_t* verdicts_dev_out);
int mpvss_ec_verify_shares_absorb(mpvss_ctx* ctx, uint8_t* verdicts_host);
/* group part of src/participant.rs:1094-1274 (secp256k1), 1573-1717 (ristretto255); randomness is input */
int mpvss_ec_distribute(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                        const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values,
                        const uint8_t* witnesses, size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out,
                        uint8_t* a2_out, uint8_t* digest32_out);
/* The same as a block (the verifier's slots, staging layout and absorbing hash; mpvss_ec_transcript_verdict(state, zero
 * challenge) yields the dealer's digest): compute enqueues, absorb waits, validates, hashes and hands out X, Y, a1, a2.
 * commitments == NULL: X_i = P(i) * G through the fixed-base comb (the dealer knows the polynomial; positions unused).
 * *_dev_out (MPVSS_DEVICE only, optional): the results also stay in HBM. */
int mpvss_ec_distribute_compute(mpvss_ctx* ctx, int group, int space, const uint8_t* commitments, size_t t,
                                const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values,
                                const uint8_t* witnesses, size_t n, uint8_t* x_dev_out, uint8_t* y_dev_out,
                                uint8_t* a1_dev_out, uint8_t* a2_dev_out);
int mpvss_ec_distribute_absorb(mpvss_ctx* ctx, uint8_t* state, uint8_t* x_out_host, uint8_t* y_out_host,
                               uint8_t* a1_out_host, uint8_t* a2_out_host);
/* The curve groups' dealer with the SCALAR side on the device as well (src/participant.rs:1134-1168, 1200-1230 secp256k1;
 * 1607-1631, 1662-1690 ristretto255) -- the counterparts of mpvss_modp_poly_eval_device / _dleq_responses_device / _deal_compute /
 * _deal.  Scalars are 32 bytes in the group's byte order; positions enter as `position as u64`, as in the reference.
 *   poly_eval_device     out_dev[i] = P(positions_dev[i]) mod order (t coefficients from the host, Horner's rule, one share per lane)
 *   dleq_responses_device r_dev_out[i] = w_dev[i] - alpha_dev[i] c mod order (one shared challenge from the host)
 *   deal_compute         one dealer's block with P(i) evaluated on the block's own stream into p_dev_out (kept for the responses),
 *                        then as mpvss_ec_distribute_compute with commitments == NULL; absorbed by mpvss_ec_distribute_absorb
 *   deal                 the whole box in one call from HOST buffers: P(i), X_i, Y_i, a1_i, a2_i, digest, challenge, responses;
 *                        x_out, a1_out, a2_out, digest32_out, challenge_out32 are optional; t <= n.  One deal at a time per context;
 *                        P(i), the witnesses and the coefficients are zeroed on the device before it returns. */
/* a curve-group block taken by mpvss_block_claim: waits for and hashes exactly that block (cf. mpvss_modp_verify_block_absorb_claimed) */
int mpvss_ec_block_absorb_claimed(mpvss_ctx* ctx, unsigned long long ticket, uint8_t* state, uint8_t* x_out_host,
                                  uint8_t* y_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host);
int mpvss_ec_poly_eval_device(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                              size_t n, uint8_t* out_dev);
int mpvss_ec_dleq_responses_device(mpvss_ctx* ctx, int group, const uint8_t* w_dev, const uint8_t* alpha_dev,
                                   const uint8_t* c_host32, size_t n, uint8_t* r_dev_out);
int mpvss_ec_deal_compute(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                          const uint8_t* pubkeys_dev, const uint8_t* witnesses_dev, size_t n, uint8_t* p_dev_out,
                          uint8_t* x_dev_out, uint8_t* y_dev_out, uint8_t* a1_dev_out, uint8_t* a2_dev_out);
int mpvss_ec_deal(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                  const uint8_t* pubkeys_host, const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out,
                  uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out32, uint8_t* r_out);

/* Key sets of a curve group.  The dealer's Y_i = P(i) y_i and a2_i = w_i y_i are multiples of long-lived public keys.  A key
 * set holds, for each of n keys, the fixed-base comb the context keeps for the generator: rows[key][w][i] = (i + 1) 16^w y_key,
 * w < 65, i < 8, packed affine entries of 64 (secp256k1) / 96 (ristretto255) bytes -- 33 280 / 49 920 bytes per key plus one
 * mark byte, mpvss_ec_keyset_bytes_per_key; 65 536 keys take 2.2 / 3.3 GB.  Over the rows k y is 65 mixed additions and no
 * doublings, against 128 doublings + about 66 additions (secp256k1, endomorphism) or 256 + 64 (ristretto255) over a table built
 * per call; the key's decode (a field square root) and table build disappear from every call.
 * KEYS: canonical encodings of 33 / 32 bytes.  One invalid encoding refuses the whole create with MPVSS_E_INVALID, the smallest
 * bad index named by mpvss_last_error, *out = NULL.  The identity (33 / 32 zero bytes) is a valid key: it has no affine form
 * on secp256k1, so the set marks such a key and every multiple of it comes out as the identity.
 * OWNERSHIP: a set belongs to the context that built it, remembers its curve and never changes.  destroy synchronises the
 * set's context first (a block enqueued by mpvss_ec_deal_compute_keyset may still read the rows) and frees the set on its own
 * context whichever context is named (both arguments may be null); a set is destroyed before its context.
 * ERRORS: MPVSS_E_INVALID for a set of another context or of the other curve, for key_offset + n beyond the set, for a scalar
 * that is not below the group order (its index named) and for create with n == 0 or a null pointer; an allocation that fails is
 * MPVSS_E_NOMEM and leaves the context usable.  n == 0 behaves as in the calls that take the keys as an array.
 * RESULTS are byte-identical to those calls -- mpvss_ec_batch_exp, a2 of mpvss_ec_dleq_commitments, mpvss_ec_deal_compute
 * followed by mpvss_ec_distribute_absorb, mpvss_ec_deal with digest, challenge and responses -- with pubkeys = the keys
 * key_offset .. key_offset + n - 1 of the set.  The rows hold public values only and are not wiped; P(i), the witnesses and
 * the coefficients are wiped exactly as in those calls.
 * Not offered: verify_distribution, verify_many and distribute over a key set (a2 = r y + c Y of the verifier still needs the
 * doublings for the fresh Y); a key cache behind the calls that take a key array; a half-size secp256k1 set through the
 * endomorphism (33 windows, the entries of phi(y) by one product with beta) -- the follow-up if memory matters; any automatic
 * routing: the caller builds the set and names it. */
typedef struct mpvss_ec_keyset mpvss_ec_keyset;
/* bytes of one key in a set of this curve: its rows and its mark; host only; 0 for an unknown group */
size_t mpvss_ec_keyset_bytes_per_key(int group);
/* pubkeys: n encodings in `space`; the build is 256 doublings per key and, per window, 4 doublings, 3 additions and ONE field
 * inversion for the eight entries */
int mpvss_ec_keyset_create(mpvss_ctx* ctx, int group, int space, const uint8_t* pubkeys, size_t n, mpvss_ec_keyset** out);
void mpvss_ec_keyset_destroy(mpvss_ctx* ctx, mpvss_ec_keyset* keyset);
/* device bytes of the set; host only; 0 for no set */
size_t mpvss_ec_keyset_bytes(const mpvss_ec_keyset* keyset);
/* out1[i] = e1[i] y_(key_offset+i), out2[i] = e2[i] y_(key_offset+i): two scalar sets in one launch; e2 and out2 may both be
 * NULL (one power).  Scalars: 32 bytes each in the group's byte order, in `space`, as the outputs */
int mpvss_ec_keyset_twin_exp(mpvss_ctx* ctx, int group, int space, const mpvss_ec_keyset* keyset, size_t key_offset,
                             const uint8_t* e1, const uint8_t* e2, size_t n, uint8_t* out1, uint8_t* out2);
/* out[i] = e1[i] y_(key_offset+i) + e2[i] h2[i]; h2 == NULL: the first term alone.  e2: n scalars in `space` when
 * e2_per_share, else ONE scalar in host memory for every share (as c of mpvss_ec_dleq_commitments).  The shape of the
 * verifier's a2, as a building block: the walk, the one-table window kernel for h2, an addition, the encode */
int mpvss_ec_keyset_dual_exp(mpvss_ctx* ctx, int group, int space, const mpvss_ec_keyset* keyset, size_t key_offset,
                             const uint8_t* e1, const uint8_t* h2, const uint8_t* e2, int e2_per_share, size_t n, uint8_t* out);
/* mpvss_ec_deal_compute with (keyset, key_offset) in place of pubkeys_dev; absorbed by mpvss_ec_distribute_absorb */
int mpvss_ec_deal_compute_keyset(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev,
                                 const mpvss_ec_keyset* keyset, size_t key_offset, const uint8_t* witnesses_dev, size_t n,
                                 uint8_t* p_dev_out, uint8_t* x_dev_out, uint8_t* y_dev_out, uint8_t* a1_dev_out,
                                 uint8_t* a2_dev_out);
/* mpvss_ec_deal with (keyset, key_offset) in place of pubkeys_host: no key upload, decode or table build */
int mpvss_ec_deal_keyset(mpvss_ctx* ctx, int group, const uint8_t* coeffs_host, size_t t, const int64_t* positions_host,
                         const mpvss_ec_keyset* keyset, size_t key_offset, const uint8_t* witnesses_host, size_t n, uint8_t* x_out,
                         uint8_t* y_out, uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out32,
                         uint8_t* r_out);
/* since the context was created, both curves together: the keys whose rows were built, and the multiples k y computed by a walk
 * over rows (two per share of a dealer's block or a twin call with e2, one otherwise); either pointer may be NULL */
int mpvss_ec_keyset_stats(mpvss_ctx* ctx, unsigned long long* keys_built, unsigned long long* powers_from_rows);

/* Group::hash_to_scalar(data), host only; out32 in the group's scalar byte order */
int mpvss_ec_hash_to_scalar(int group, const uint8_t* data, size_t len, uint8_t out32[32]);

/* ---- extract_secret_share, batched (the callers on the other side of the path) --------------------------------
 * n participants decrypt their encrypted share and build the DLEQ proof at once, src/participant.rs:294-353
 * (secp256k1 :1282-1338, ristretto255 :1725-1781):  S_i = Y_i^(1/x_i),  a1_i = G^w_i,  a2_i = S_i^w_i,
 * c_i = hash_to_scalar(SHA256(framed(pk_i) framed(Y_i) framed(a1_i) framed(a2_i))).
 * xinv = x_i^-1 mod the group order (host work: util.rs:33-41 / Scalar::invert) and the witnesses w are inputs;
 * the response r_i = w_i - x_i c_i (dleq.rs:42-50) stays with the host.  s_out in `space`; c_out_host: n scalars. */
int mpvss_modp_extract_shares(mpvss_ctx* ctx, int space, const uint8_t* pk, const uint8_t* y, const uint8_t* xinv,
                              const uint8_t* w, size_t n, uint8_t* s_out, uint8_t* c_out_host);
int mpvss_ec_extract_shares(mpvss_ctx* ctx, int group, int space, const uint8_t* pk, const uint8_t* y,
                            const uint8_t* xinv, const uint8_t* w, size_t n, uint8_t* s_out, uint8_t* c_out_host);
/* MODP, in two steps, so that several batches are in flight (they share the MPVSS_BLOCK_SLOTS block slots and the FIFO order of
 * the other block calls): `compute` forms e2 = w / x mod (q-1) on host threads and only ENQUEUES the GPU work -- S and a2 from
 * one chain of squarings, a1 through the comb, and the challenge hash of every proof on the device (K7) --, `absorb` waits for
 * the oldest batch and hands out S and c (n x 256 bytes each).  Host buffers.  A batch with an encrypted share that is 0 mod q
 * (no group element) is refused with MPVSS_E_UNSUPPORTED: it belongs to mpvss_modp_extract_shares. */
int mpvss_modp_extract_shares_compute(mpvss_ctx* ctx, const uint8_t* pk, const uint8_t* y, const uint8_t* xinv, const uint8_t* w,
                                      size_t n);
int mpvss_modp_extract_shares_absorb(mpvss_ctx* ctx, uint8_t* s_out_host, uint8_t* c_out_host);

/* ---- scalar-field side (host only, no context needed) ------------------------------------------------------------
 * The reference's scalar rings: Z/(q-1) for MODP-2048 (256-byte big-endian scalars), Z/n for secp256k1 (32-byte
 * big-endian), Z/l for ristretto255 (32-byte little-endian).  O(n) / O(n t) word operations per box against O(3000 n)
 * 2048-bit products on the group side: threaded over the shares on the host (threads <= 0: up to 16). */
/* Group::scalar_mul: (a * b) % order        src/group.rs:108, modp.rs:180-182, secp256k1.rs:173-176, ristretto255.rs:244-247 */
int mpvss_modp_scalar_mul(const uint8_t* a256, const uint8_t* b256, uint8_t* out256);
int mpvss_ec_scalar_mul(int group, const uint8_t* a32, const uint8_t* b32, uint8_t* out32);
/* Group::scalar_sub: a - b normalised into [0, order)   src/group.rs:113, modp.rs:184-192, secp256k1.rs:178-181 */
int mpvss_modp_scalar_sub(const uint8_t* a256, const uint8_t* b256, uint8_t* out256);
int mpvss_ec_scalar_sub(int group, const uint8_t* a32, const uint8_t* b32, uint8_t* out32);
/* r[i] = w[i] - alpha[i] * c_i (mod order): Prover::response / DLEQ::get_r (src/dleq.rs:42-50,221-228) for n proofs --
 * the dealer's responses (participant.rs:255-264: alpha = P(i), one shared c) and the participants'
 * (participant.rs:345-350: alpha = private key, c per share).  c: one scalar (c_per_share == 0) or n. */
int mpvss_modp_dleq_responses(const uint8_t* w, const uint8_t* alpha, const uint8_t* c, int c_per_share, size_t n,
                              uint8_t* r_out, int threads);
int mpvss_ec_dleq_responses(int group, const uint8_t* w, const uint8_t* alpha, const uint8_t* c, int c_per_share, size_t n,
                            uint8_t* r_out, int threads);
/* out[i] = P(positions[i]) mod order for P = sum_j coeffs[j] x^j: Polynomial::get_value (src/polynomial.rs:50-58) followed
 * by the caller's `% order` (participant.rs:202, 1155-1157, 1619-1621).  MODP positions must be >= 0. */
int mpvss_modp_poly_eval(const uint8_t* coeffs, size_t t, const int64_t* positions, size_t n, uint8_t* out, int threads);
int mpvss_ec_poly_eval(int group, const uint8_t* coeffs, size_t t, const int64_t* positions, size_t n, uint8_t* out, int threads);
/* The MODP pair on the DEVICE (2048-bit scalars: the host loops above cost more than the group work of a box): P(i) for
 * positions in HBM (>= 0) from the dealer's coefficients in host memory, results in HBM as 256-byte big-endian scalars in
 * [0, q-1) (what mpvss_modp_distribute_compute takes as p_values); and r[i] = w[i] - alpha[i] c mod (q-1) for ONE shared c
 * (host), w, alpha and r in HBM.  Same values as the host functions (src/polynomial.rs:50-58, src/dleq.rs:42-50);
 * synchronous: the results are complete when the call returns. */
int mpvss_modp_poly_eval_device(mpvss_ctx* ctx, const uint8_t* coeffs_host, size_t t, const int64_t* positions_dev, size_t n,
                                uint8_t* out_dev);
int mpvss_modp_dleq_responses_device(mpvss_ctx* ctx, const uint8_t* w_dev, const uint8_t* alpha_dev, const uint8_t* c_host, size_t n,
                                     uint8_t* r_dev_out);

/* ---- reconstruct ---------------------------------------------------------------------------------------------------
 * G^s = prod_i S_i^lambda_i from m >= t decrypted shares S_i at pairwise different positions (host int64):
 * src/participant.rs:462-561 (MODP; positions >= 1 as util.rs:47-64 assumes), 1452-1557 (secp256k1), 1895-2002
 * (ristretto255).  A position below 1 is MPVSS_E_INVALID in all three groups: a box's positions are 1..n.  Lagrange
 * coefficients in the scalar field on the host, the m exponentiations and their product on the GPU.  gs_out: G^s (256 / 33 / 32 bytes); mask_out32 (optional): the 32-byte big-endian mask the reference XORs
 * onto U -- int_BE(SHA256(bytes(G^s))) mod q / mod n / mod l (participant.rs:512-517, 1495-1511, 1939-1949):
 * secret = mask XOR U.  shares in `space`. */
int mpvss_modp_reconstruct(mpvss_ctx* ctx, int space, const int64_t* positions_host, const uint8_t* shares, size_t m,
                           uint8_t* gs_out256, uint8_t* mask_out32);
int mpvss_ec_reconstruct(mpvss_ctx* ctx, int group, int space, const int64_t* positions_host, const uint8_t* shares, size_t m,
                         uint8_t* gs_out, uint8_t* mask_out32);

/* Many secrets of a curve group in one call: the contract of mpvss_modp_group_reconstruct_many (below, run-time MODP groups) with
 * the group's encoding length L (33 / 32) as the element size.  For every secret i that mpvss_ec_reconstruct accepts,
 * status[i] == MPVSS_OK and gs_out[i L .. i L + L - 1] and masks_out32[32 i .. 32 i + 31] (optional) are what that call gives for
 * (positions_host, shares, m) on the same context, byte for byte, in both spaces and for both curves; in device space the share
 * buffers are left unchanged.  The Lagrange coefficients are computed once per distinct position list of the call (lists are equal
 * when their sequences are: a permuted list is another list).  Runs of consecutive secrets of at most 16384 shares each travel
 * through the GPU as one batch of at most MPVSS_MAX_CHUNK shares, one wave per secret for the sum; every longer secret, and a run
 * of one, takes the one-secret path.
 * shares live in `space`; positions_host, secrets, status, gs_out and masks_out32 are host memory.  The call is synchronous and
 * holds the context lock like its one-secret sibling.  host_threads: up to that many host threads compute the Lagrange
 * coefficients and the masks (clamped to 1..16; <= 0: the library chooses from the work of the call, at most 16, never by the
 * machine's CPU count).
 * ERRORS: no context is MPVSS_E_INVALID, an unknown group MPVSS_E_UNSUPPORTED; count == 0 is MPVSS_OK; secrets, status or gs_out
 * NULL with count > 0 are MPVSS_E_INVALID; all of these write no output.  A refused secret -- whatever the one-secret call answers
 * with MPVSS_E_INVALID: a pointer NULL, m == 0, m above 0x7fffffff, a position below 1, duplicate positions, a share that is not a
 * valid encoding -- costs only itself: that code in status[i], zeros in gs_out[i] and in its mask, and the call goes on and returns
 * MPVSS_OK.  A HIP error or a failed allocation ends the call with the code the one-secret call returns and leaves the context
 * usable.
 * mpvss_ec_reconstruct_many_stats: since the context was created, the grouped passes, the secrets that went through them and the
 * secrets that took the one-secret path (refused secrets are in none; both curves count together); any pointer may be NULL, no
 * context is MPVSS_E_INVALID. */
typedef struct mpvss_ec_secret {
  const int64_t* positions_host;   /* m positions, host memory in either space */
  const uint8_t* shares;           /* m encoded elements (33 / 32 bytes each), in `space` */
  size_t m;
} mpvss_ec_secret;
int mpvss_ec_reconstruct_many(mpvss_ctx* ctx, int group, int space, const mpvss_ec_secret* secrets, size_t count,
                              int host_threads, int* status, uint8_t* gs_out, uint8_t* masks_out32);
int mpvss_ec_reconstruct_many_stats(mpvss_ctx* ctx, unsigned long long* passes, unsigned long long* grouped_secrets,
                                    unsigned long long* single_secrets);

/* Where mpvss_ec_reconstruct and mpvss_ec_reconstruct_many compute the Lagrange coefficients lambda_i = prod_{j != i} x_j / (x_j - x_i)
 * mod the group order (participant.rs:1518-1557, 1955-2002): mode 0 on the host as before, 2 on the device (k_ec_lagrange: one
 * coefficient per lane, one launch for all distinct position lists of a call, the scalars never cross the bus) whenever the lists
 * allow it -- no list of more than 2^20 positions, fewer than 2^31 positions in all -- and 1, the default, on the device when the work
 * of the call (the sum of m^2 over its distinct lists; m^2 of a lone secret) reaches a measured size ("Lagrange
 * coefficients on the device, curve groups"; profiles/ec_lagrange_device.txt).  A coefficient is one element of a prime field, so
 * the results of all four reconstruct entry points are the same bytes under every mode.  Returns the mode before; no context, or
 * another value, is MPVSS_E_INVALID. */
int mpvss_ctx_set_ec_lagrange(mpvss_ctx* ctx, int mode);
/* The kernel on its own: scalars_out_host[32 i .. 32 i + 31] = the scalar share i of a secret at these positions is multiplied by,
 * lambda_i mod the order ("order - |lambda_i|" for a negative coefficient) in the group's scalar byte order (secp256k1 big-endian,
 * ristretto255 little-endian), computed where the context's mode says.  Refusals are those of mpvss_ec_reconstruct: a NULL pointer,
 * m == 0, m above 0x7fffffff, a position below 1, duplicate positions are MPVSS_E_INVALID and leave the output untouched; an unknown
 * group is MPVSS_E_UNSUPPORTED.  Synchronous, under the context lock. */
int mpvss_ec_lagrange_scalars(mpvss_ctx* ctx, int group, const int64_t* positions_host, size_t m, uint8_t* scalars_out_host);
/* Position lists whose coefficients were computed on the device / on the host since the context was created, by any of the three
 * calls above (a list shared by several secrets of one call counts once; refused lists are in neither count; both curves count
 * together).  Either pointer may be NULL; no context is MPVSS_E_INVALID. */
int mpvss_ec_lagrange_stats(mpvss_ctx* ctx, unsigned long long* device_lists, unsigned long long* host_lists);

/* ---- flat wire format of a DistributionSharesBox ("MPVSSBX1") ---------------------------------------------------------
 * The reference keeps a box as three HashMap<Vec<u8>, _> (src/sharebox.rs:74-86) and defines no serialisation.  This
 * format is the boundary's own layout -- rows in `publickeys` order (the order src/participant.rs:408-448 iterates in),
 * fixed-width encodings -- so that a box can be handed to the engine, or cut into byte ranges for the ranks of a sharded
 * verification, without rebuilding maps.  Integers little-endian; every section starts at a multiple of 8 bytes
 * (zero padding, checked by the parser: an accepted buffer is its own serialisation); E = element bytes (256 / 33 / 32),
 * S = scalar bytes (256 / 32 / 32):
 *   0  "MPVSSBX1"   8  u32 group (0 MODP-2048, 1 secp256k1, 2 ristretto255)   12  u32 E   16  u64 n   24  u64 t
 *   32 u64 u_len    40 commitments [t][E] | positions i64 [n] | publickeys [n][E] | shares [n][E] | responses [n][S] |
 *   challenge [S] | U (big-endian magnitude, u_len bytes).                          (full specification: INTEGRATION.md) */
typedef struct mpvss_box_view {
  int group;
  size_t element_bytes, scalar_bytes, n, t, u_len;
  const uint8_t* commitments;
  const int64_t* positions;
  const uint8_t *pubkeys, *shares, *responses, *challenge, *u_be;
} mpvss_box_view;
size_t mpvss_box_wire_size(int group, size_t n, size_t t, size_t u_len);     /* 0: unknown group or absurd sizes */
int mpvss_box_serialize(int group, const uint8_t* commitments, size_t t, const int64_t* positions, const uint8_t* pubkeys,
                        const uint8_t* shares, const uint8_t* responses, size_t n, const uint8_t* challenge,
                        const uint8_t* u_be, size_t u_len, uint8_t* out, size_t out_cap, size_t* out_len);
/* Zero-copy view into `buf` (which must be 8-byte aligned and stay alive); rejects anything that is not exactly one box. */
int mpvss_box_parse(const uint8_t* buf, size_t len, mpvss_box_view* view);
/* verify_distribution_shares of a serialized box in host memory (any of the three groups) */
int mpvss_box_verify_wire(mpvss_ctx* ctx, const uint8_t* buf, size_t len, int* verdict, uint8_t* digest32_out);

/* ---- MODP groups of a run-time modulus (ModpGroup::init, src/groups/modp.rs:72-84) ---------------------------
 * A group handle holds an odd modulus q of at most 4096 bits -- ModpGroup::init(length).modulus() or any other -- and
 * what the kernels need of it (Montgomery constants, the width: 5, 9 or 18 limbs of 29 bits per lane, the smallest with
 * bits(q) <= 29 * 4 * limbs - 2, or 27 for a 384-byte handle and 36 for a 512-byte one).  Creating it is host work only (no GPU, no context); it is
 * immutable afterwards and may be used from any number of contexts and threads at once.
 * ELEMENT SIZE: every element, scalar and exponent that a mpvss_modp_group_* entry point reads or writes is a big-endian
 * value of mpvss_modp_group_elem_bytes(handle) bytes, and arrays of them have that stride: 256 (MPVSS_MODP_BYTES) for a
 * handle of mpvss_modp_group_create; 384 (moduli of 2049 .. 3072 bits, RFC 3526 group 15 among them) or 512 (moduli of 3073 ..
 * 4096 bits, RFC 3526 group 16 among them) for a handle of mpvss_modp_group_create_wide.  Parameter names and comments below that say 256 mean that size.  Inputs need not be reduced (a value >= q gives what BigInt::modpow / (a * b) % q give, modp.rs:154-156
 * validates nothing), outputs are canonical (< q).  The group's generators are those of ModpGroup: G = 2, g = G^2 = 4.
 * Protocol parity is specified for safe primes, which is what ModpGroup::init yields; for another odd q the calls return
 * without fault and are deterministic.
 * The entry points below mirror the group-14 ones with the handle added, lock the context like them and are safe for
 * concurrent callers on one context in the same sense.  The whole protocol is there: verification, the dealer (distribute,
 * the one-call deal), extract_secret_share and reconstruct.  The scalar ring Z/(q-1) -- P(i), the responses, e2 = w / x -- runs
 * on host threads or, for a handle with odd (q-1)/2 >= 3 (every safe prime above 5), on the device: mpvss_ctx_set_rt_scalar and
 * "the scalar ring on the device" below.  Long-lived public keys can be registered as a key set ("Key sets of a run-time group"
 * below), the boxes of a whole round verified in one call ("Many boxes in one call" below) and the secrets of a whole round
 * reconstructed in one call ("Many secrets in one call" below).  Not offered for a
 * run-time group: the block / pipeline forms, the wire format, and the overlap of one run's hashing with the next run's GPU
 * work; moduli above 4096 bits are refused
 * with MPVSS_E_INVALID (a 512-byte handle's product carries each 64-bit column accumulator once more per lane than the narrower
 * ones, DESIGN section 13, "Handles of 512 bytes"; its rates are unmeasured). */
typedef struct mpvss_modp_group mpvss_modp_group;
/* q_be: q_len big-endian bytes (leading zeros allowed).  MPVSS_E_INVALID for an even q, q < 5 or q >= 2^2048. */
int mpvss_modp_group_create(const uint8_t* q_be, size_t q_len, mpvss_modp_group** out);
/* The same with the element size chosen: elem_bytes 256 is mpvss_modp_group_create itself; 384 takes an odd q of 2049 .. 3072
 * bits and gives a handle that always runs at 27 limbs per lane; 512 takes an odd q of 3073 .. 4096 bits and gives a handle
 * that always runs at 36 limbs per lane.  A narrower q with 384 or 512 is MPVSS_E_INVALID: the next smaller handle serves it.
 * Any other elem_bytes is MPVSS_E_INVALID.  Everything a 256-byte handle can do, a 384- and a 512-byte handle can do. */
int mpvss_modp_group_create_wide(const uint8_t* q_be, size_t q_len, size_t elem_bytes, mpvss_modp_group** out);
void mpvss_modp_group_destroy(mpvss_modp_group* grp);
/* bit length of q, the limbs per lane of the width the kernels run at (5, 9, 18, 27 or 36), and the element size (256, 384 or 512) */
int mpvss_modp_group_bits(const mpvss_modp_group* grp);
int mpvss_modp_group_limbs_per_lane(const mpvss_modp_group* grp);
int mpvss_modp_group_elem_bytes(const mpvss_modp_group* grp);
/* Group::hash_to_scalar: int_BE(SHA256(data)) mod (q-1)/2, big-endian, left-padded to the element size
 * (src/groups/modp.rs:142-148); host only */
int mpvss_modp_group_hash_to_scalar(const mpvss_modp_group* grp, const uint8_t* data, size_t len, uint8_t* out256);
/* out[i] = bases[i]^exps[i] mod q                                    ModpGroup::exp (src/groups/modp.rs:122-128) */
int mpvss_modp_group_batch_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* bases, const uint8_t* exps,
                               size_t n, uint8_t* out);
/* out[i] = a[i] * b[i] mod q                                         ModpGroup::mul (src/groups/modp.rs:130-132) */
int mpvss_modp_group_batch_mul(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* a, const uint8_t* b, size_t n,
                               uint8_t* out);
/* X[i] = prod_{j<t} C_j^(positions[i]^j mod (q-1)) mod q           src/participant.rs:423-434 (as mpvss_modp_commit_eval) */
int mpvss_modp_group_commit_eval(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments, size_t t,
                                 const int64_t* positions, size_t n, uint8_t* x_out);
/* a1[i] = g1^r[i] h1[i]^c_i, a2[i] = g2[i]^r[i] h2[i]^c_i          src/dleq.rs:66-84 (as mpvss_modp_dleq_commitments) */
int mpvss_modp_group_dleq_commitments(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* g1_host, const uint8_t* h1,
                                      const uint8_t* g2, const uint8_t* h2, const uint8_t* r, const uint8_t* c, int c_per_share,
                                      size_t n, uint8_t* a1_out, uint8_t* a2_out);
/* whole-box verification, src/participant.rs:399-455: same contract as mpvss_modp_verify_distribution (verdict, digest of the
 * transcript, optional host dumps of X, a1, a2; n == 0 hashes the empty transcript) */
int mpvss_modp_group_verify_distribution(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments, size_t t,
                                         const int64_t* positions, const uint8_t* pubkeys, const uint8_t* shares,
                                         const uint8_t* responses, size_t n, const uint8_t* challenge_host, int* verdict,
                                         uint8_t* digest32_out, uint8_t* x_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host);
/* n share-box proofs, src/participant.rs:361-386 -> src/dleq.rs:275-302 (as mpvss_modp_verify_shares); products on the GPU, the
 * per-share hashes on the host or on the device (mpvss_ctx_set_rt_share_hash below; the same verdicts either way -- on the
 * device a1 and a2 stay there and one verdict byte per share crosses the bus) */
int mpvss_modp_group_verify_shares(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* pk, const uint8_t* s,
                                   const uint8_t* y, const uint8_t* c, const uint8_t* r, size_t n, uint8_t* verdicts_host);

/* out1[i] = bases[i]^e1[i], out2[i] = bases[i]^e2[i] mod q: two powers of one base per share, the shape of the dealer's
 * (Y_i, a2_i) = (y_i^P(i), y_i^w_i) and the participant's (S_i, a2_i) = (Y_i^(1/x_i), Y_i^(w_i/x_i)).  Large batches share the
 * squarings (right to left over 4-bit windows into buckets in HBM, zeroed before the call returns); small ones run two
 * left-to-right exponent sets in one launch.  Same bytes either way.  All arrays n x 256 bytes in `space`. */
int mpvss_modp_group_batch_twin_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* bases, const uint8_t* e1,
                                    const uint8_t* e2, size_t n, uint8_t* out1, uint8_t* out2);
/* the batch size (shares of one call, or of one chunk of a longer one) from which this group's width takes the shared-squarings
 * kernel; smaller batches run the two exponent sets.  Host only; informational -- the results do not depend on it. */
int mpvss_modp_group_twin_min_shares(const mpvss_modp_group* grp);
/* out[i] = base^exps[i] mod q for ONE base in host memory (256 bytes, any value): the handle's counterpart of
 * mpvss_modp_batch_exp_fixed_base -- generate_public_key (base G = 2) and the commitments C_j = g^a_j (base g = 4).  exps and out
 * n x 256 bytes in `space`; exponents staged from the host are zeroed on the device before the call returns.
 * Fixed-base combs: a context keeps up to 4 tables base^(d 16^k), k < 2 x element size, d < 16, keyed by the bytes (q, base), least recently
 * used evicted, freed with the context.  Every power of a base shared by a whole call -- this entry point, X_i = g^P(i) and
 * a1_i = g^w_i of group_deal / group_distribute, a1_i = G^w_i of group_extract_shares, the g1^r leg of a1 in
 * group_dleq_commitments / group_verify_distribution / group_verify_shares -- runs over the comb without squarings when the
 * context has it, builds it when the call (or chunk) has at least mpvss_modp_group_comb_min_shares shares, and otherwise takes
 * the 16-entry window table as before.  Same bytes either way.  The tables hold public values only. */
int mpvss_modp_group_batch_exp_fixed_base(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* base_host,
                                          const uint8_t* exps, size_t n, uint8_t* out);
/* builds the combs of the group's generators g = 4 and G = 2 on this context now, so that small calls use them too */
int mpvss_modp_group_prepare(mpvss_ctx* ctx, const mpvss_modp_group* grp);
/* the batch size from which a call builds a comb it does not find in the context's cache.  Host only; informational -- the
 * results do not depend on it. */
int mpvss_modp_group_comb_min_shares(const mpvss_modp_group* grp);
/* comb cache of the context since it was created: tables built, uses of a cached table, tables evicted (any pointer may be null) */
int mpvss_modp_group_comb_stats(mpvss_ctx* ctx, unsigned long long* builds, unsigned long long* hits, unsigned long long* evictions);
/* Forward differences in the exponent for X_i of a run-time group (commit_eval, verify_distribution, distribute with commitments):
 * t - 1 products per share instead of Horner's rule, taken per chunk when the positions are consecutive from p0 >= 0 and all below
 * q - 1, every commitment is a unit mod q, 2 <= t <= fd_max_t and the chunk has at least fd_min_shares(t) shares.  The results
 * are the same bytes either way.  mode 0: off; 1: automatic (the default); 2: whenever admissible, whatever fd_min_shares says.
 * chains 0: automatic; another value is clamped so that every chain holds at least t positions. */
int mpvss_ctx_set_rt_fd(mpvss_ctx* ctx, int mode, int chains);
/* the chunk size from which mode 1 takes forward differences at this t, and the largest t they serve.  Host only. */
int mpvss_modp_group_fd_min_shares(const mpvss_modp_group* grp, size_t t);
int mpvss_modp_group_fd_max_t(const mpvss_modp_group* grp);
/* chunks of X_i computed by forward differences and by Horner's rule since the context was created (either pointer may be null) */
int mpvss_modp_group_fd_stats(mpvss_ctx* ctx, unsigned long long* fd_calls, unsigned long long* horner_calls);
/* dealer's group side, src/participant.rs:160-286 with p_i = P(i) mod (q-1) and the witnesses as input: same contract as
 * mpvss_modp_distribute */
int mpvss_modp_group_distribute(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments, size_t t,
                                const int64_t* positions, const uint8_t* pubkeys, const uint8_t* p_values, const uint8_t* witnesses,
                                size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out);
/* the dealer's whole box in one call from HOST buffers: same contract as mpvss_modp_deal (x_out, a1_out, a2_out, digest32_out
 * and challenge_out256 optional; t <= n; t == 0 with n > 0 and a negative position are MPVSS_E_INVALID; n == 0 gives the digest
 * of the empty transcript).  P(i) and the responses are host-thread work or run on the device (mpvss_ctx_set_rt_scalar; the same
 * bytes either way; on the device P(i), w and the responses of all n shares stay in HBM until the call ends, 3 n x the element size in bytes), X_i = g^P(i) and a1_i = g^w_i run over the
 * comb of g = 4, or over its window table for a small box on a context without the comb.  Every buffer of the call that held coefficients, P(i), witnesses or buckets is zeroed before it
 * returns, on error paths too. */
int mpvss_modp_group_deal(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t,
                          const int64_t* positions_host, const uint8_t* pubkeys_host, const uint8_t* witnesses_host, size_t n,
                          uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out, uint8_t* a2_out, uint8_t* digest32_out,
                          uint8_t* challenge_out256, uint8_t* r_out);
/* n participants' extract_secret_share, src/participant.rs:294-353: same contract as mpvss_modp_extract_shares (xinv = x^-1 mod
 * (q-1) and the witnesses are inputs; the per-share challenge is hashed on the host or on the device, mpvss_ctx_set_rt_share_hash below,
 * the same bytes either way).  A row whose Y_i is 0 mod q gives the
 * reference's values (S_i = 0, a2_i = 0^w_i).  e2_i = w_i xinv_i mod (q-1) is formed on host threads or on the device
 * (mpvss_ctx_set_rt_scalar), the same bytes either way. */
int mpvss_modp_group_extract_shares(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* pk, const uint8_t* y,
                                    const uint8_t* xinv, const uint8_t* w, size_t n, uint8_t* s_out, uint8_t* c_out_host);
/* G^s and the mask from m shares, src/participant.rs:462-561: same contract as mpvss_modp_reconstruct (positions >= 1 and pairwise
 * different; a Lagrange coefficient whose denominator, with the fraction in lowest terms as the reference takes it (:546-553),
 * has no inverse mod (q-1)/2, an even (q-1)/2, or a share that is 0 mod q where its factor has to be inverted gives
 * MPVSS_E_INVALID).  A raw denominator that is 0 mod a small (q-1)/2 is no refusal by itself: q = 23 with positions {1, 11, 12}
 * has 132/110 = 6/5 mod 11.  mask_out32 = int_BE(SHA256(minimal bytes(G^s))) mod q, 32 bytes big-endian. */
int mpvss_modp_group_reconstruct(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const int64_t* positions_host,
                                 const uint8_t* shares, size_t m, uint8_t* gs_out256, uint8_t* mask_out32);
/* the scalar ring Z/(q-1) of the handle (host only, no context): the contracts of mpvss_modp_scalar_mul, _scalar_sub,
 * _dleq_responses and _poly_eval -- 256-byte big-endian scalars, inputs need not be reduced, threads <= 0: up to 16 */
int mpvss_modp_group_scalar_mul(const mpvss_modp_group* grp, const uint8_t* a256, const uint8_t* b256, uint8_t* out256);
int mpvss_modp_group_scalar_sub(const mpvss_modp_group* grp, const uint8_t* a256, const uint8_t* b256, uint8_t* out256);
int mpvss_modp_group_dleq_responses(const mpvss_modp_group* grp, const uint8_t* w, const uint8_t* alpha, const uint8_t* c,
                                    int c_per_share, size_t n, uint8_t* r_out, int threads);
int mpvss_modp_group_poly_eval(const mpvss_modp_group* grp, const uint8_t* coeffs, size_t t, const int64_t* positions, size_t n,
                               uint8_t* out, int threads);
/* The scalar ring on the device.  For odd q' = (q-1)/2, Z/(q-1) = Z/2 x Z/q': the kernels keep a scalar as its residue mod q'
 * (Montgomery form at the handle's width, constants of q' in the handle) and its parity, and write the one number of [0, q-1)
 * with both.  mpvss_modp_group_has_device_scalar: 1 when q' is odd and >= 3 (every safe prime above 5), else 0; host only.
 * The three calls below mirror mpvss_modp_poly_eval_device, mpvss_modp_dleq_responses_device and mpvss_modp_scalar_mul per share,
 * with the handle added: every scalar 256 bytes (the handle's element size) of any value, results canonical and byte-identical
 * to mpvss_modp_group_poly_eval / _dleq_responses (one shared c) / _scalar_mul.  n == 0 is MPVSS_OK; t == 0 with n > 0 and a
 * negative position (found after the fact from the copied-back positions) are MPVSS_E_INVALID; so is a handle without the
 * constants of q' -- these calls have no host path inside.  They run on the context's stream under its lock and are synchronous.
 * The staged coefficients (pinned and device copy) are zeroed on every way out; batch_scalar_mul zeroes what it staged from
 * the host. */
int mpvss_modp_group_has_device_scalar(const mpvss_modp_group* grp);
int mpvss_modp_group_poly_eval_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t,
                                      const int64_t* positions_dev, size_t n, uint8_t* out_dev);
int mpvss_modp_group_dleq_responses_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* w_dev, const uint8_t* alpha_dev,
                                           const uint8_t* c_host, size_t n, uint8_t* r_dev_out);
int mpvss_modp_group_batch_scalar_mul(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* a, const uint8_t* b,
                                      size_t n, uint8_t* out);
/* Where group_deal and group_extract_shares run the scalar ring: mode 0 on host threads; 1 automatic (the default): on the device
 * from mpvss_modp_group_scalar_min_shares shares of a whole call -- not yet measured, so until then automatic means host; 2 on
 * the device whenever the handle allows it.  A handle without the constants of q' always takes the host path. */
int mpvss_ctx_set_rt_scalar(mpvss_ctx* ctx, int mode);
int mpvss_modp_group_scalar_min_shares(const mpvss_modp_group* grp);
/* whole group_deal / group_extract_shares calls that ran the scalar ring on the device and on the host since the context was
 * created (either pointer may be null) */
int mpvss_modp_group_scalar_stats(mpvss_ctx* ctx, unsigned long long* device_calls, unsigned long long* host_calls);
/* The per-share DLEQ hash on the device.  The challenge of a share proof is hash_to_scalar(SHA256(framed(pk_i) framed(Y_i)
 * framed(a1_i) framed(a2_i))) (src/dleq.rs:87-126: framed(b) = u64-BE(len) || the minimal big-endian bytes of the element as given,
 * zero as one 0x00 byte); verify_share compares it with c_i (src/participant.rs:361-386 -> src/dleq.rs:275-302), the prover of
 * extract_secret_share hands it out (src/participant.rs:329-343).  The kernel computes int_BE(SHA256(SHA256(transcript))) and does
 * not reduce it, so a handle is admitted only where hash_to_scalar's reduction is the identity; every other handle (moduli below
 * 258 bits: test sizes) keeps the host path under every mode. */
/* 1 when (q-1)/2 >= 2^256, so hash_to_scalar is the identity on a SHA-256 output; host only */
int mpvss_modp_group_has_device_share_hash(const mpvss_modp_group* grp);
/* where group_verify_shares / group_extract_shares hash: 0 host, 1 automatic (default), 2 device whenever the handle allows.
 * Automatic takes the device at every batch size: measured no slower than the host path from the smallest size on (DESIGN
 * section 13, "Per-share hash on the device"; profiles/modp_rt_share_hash_rate.txt). */
int mpvss_ctx_set_rt_share_hash(mpvss_ctx* ctx, int mode);
/* whole calls of those two entry points that hashed on the device / on the host since the context was created */
int mpvss_modp_group_share_hash_stats(mpvss_ctx* ctx, unsigned long long* device_calls, unsigned long long* host_calls);
/* c_out[i] = hash_to_scalar(SHA256(framed(h1_i) framed(h2_i) framed(a1_i) framed(a2_i))), dleq.rs:87-126, for n transcripts;
 * all five arrays n x element size in `space`; n == 0 is MPVSS_OK; a handle without the device hash is MPVSS_E_INVALID
 * (no host path inside, as mpvss_modp_group_batch_scalar_mul) */
int mpvss_modp_group_dleq_challenges(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* h1, const uint8_t* h2,
                                     const uint8_t* a1, const uint8_t* a2, size_t n, uint8_t* c_out);

/* Key sets of a run-time group.  The full-width powers of a participant's public key -- a2_i = y_i^r_i Y_i^c of the verifier,
 * Y_i = y_i^P(i) and a2_i = y_i^w_i of the dealer -- are the largest term of a share, and keys are long-lived: a key set holds,
 * for each of n keys, the rows y^(d 2^(256 j)), j < element size / 32, d < 16 (mpvss_modp_group_keyset_bytes_per_key bytes per
 * key: 10 240, 18 432, 36 864 or 82 944 at 5, 9, 18 or 27 limbs per lane), over which such a power needs 252 squarings instead
 * of 2 044 at 2048 bits.  Keys need not be reduced; a key that is 0 mod q gives 0^0 = 1 and 0^e = 0 (modp.rs:122-128).
 * OWNERSHIP: a set belongs to the context that built it, remembers the modulus and width it was built for and never changes.
 * The calls below are synchronous, so destroying a set after the last call that named it has returned is safe; destroy frees it
 * on its own context whichever context is named (both arguments may be null); a set is destroyed before its context.
 * ERRORS: MPVSS_E_INVALID for a set of another context or another modulus, for key_offset + n beyond the set, and for create
 * with n == 0 or a null pointer; an allocation that fails is MPVSS_E_NOMEM and leaves the context usable.  RESULTS are byte-identical to the calls that take the keys as an
 * array -- a2 of mpvss_modp_group_dleq_commitments, mpvss_modp_group_batch_twin_exp, mpvss_modp_group_verify_distribution and
 * mpvss_modp_group_deal with pubkeys = the keys key_offset .. key_offset + n - 1 of the set -- n == 0, the optional dumps, the
 * digests and the challenge included, under every mode of mpvss_ctx_set_rt_scalar and mpvss_ctx_set_rt_fd.  The rows hold
 * public values only and are not wiped; exponents staged from the host are treated as in those calls.  Not offered: a key
 * cache behind the calls that take a key array, and group_distribute over a key set. */
typedef struct mpvss_modp_group_keyset mpvss_modp_group_keyset;
/* bytes of one key's rows at this handle's width; host only; 0 for no group */
size_t mpvss_modp_group_keyset_bytes_per_key(const mpvss_modp_group* grp);
/* pubkeys: n x element size bytes in `space`; the build is 1 + 256 (J - 1) + 14 J products per key, J = element size / 32 */
int mpvss_modp_group_keyset_create(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* pubkeys, size_t n,
                                   mpvss_modp_group_keyset** out);
void mpvss_modp_group_keyset_destroy(mpvss_ctx* ctx, mpvss_modp_group_keyset* keyset);
/* device bytes of the set's rows; host only; 0 for no set */
size_t mpvss_modp_group_keyset_bytes(const mpvss_modp_group_keyset* keyset);
/* out[i] = y_(key_offset+i)^e1[i] * h2[i]^e2[i] mod q; h2 == NULL: the first factor alone.  e2: n scalars in `space` when
 * e2_per_share, else ONE scalar in host memory for every share (as c of mpvss_modp_group_dleq_commitments) */
int mpvss_modp_group_keyset_dual_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_keyset* keyset,
                                     size_t key_offset, const uint8_t* e1, const uint8_t* h2, const uint8_t* e2, int e2_per_share,
                                     size_t n, uint8_t* out);
/* out1[i] = y_(key_offset+i)^e1[i], out2[i] = y_(key_offset+i)^e2[i] mod q: two exponent sets in one launch */
int mpvss_modp_group_keyset_twin_exp(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_keyset* keyset,
                                     size_t key_offset, const uint8_t* e1, const uint8_t* e2, size_t n, uint8_t* out1, uint8_t* out2);
/* mpvss_modp_group_verify_distribution with (keyset, key_offset) in place of pubkeys */
int mpvss_modp_group_verify_distribution_keyset(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* commitments,
                                                size_t t, const int64_t* positions, const mpvss_modp_group_keyset* keyset,
                                                size_t key_offset, const uint8_t* shares, const uint8_t* responses, size_t n,
                                                const uint8_t* challenge_host, int* verdict, uint8_t* digest32_out,
                                                uint8_t* x_out_host, uint8_t* a1_out_host, uint8_t* a2_out_host);
/* mpvss_modp_group_deal with (keyset, key_offset) in place of pubkeys_host */
int mpvss_modp_group_deal_keyset(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t,
                                 const int64_t* positions_host, const mpvss_modp_group_keyset* keyset, size_t key_offset,
                                 const uint8_t* witnesses_host, size_t n, uint8_t* x_out, uint8_t* y_out, uint8_t* a1_out,
                                 uint8_t* a2_out, uint8_t* digest32_out, uint8_t* challenge_out256, uint8_t* r_out);

/* Many boxes in one call.  Every participant of a PVSS round deals, so a verifier holds tens to hundreds of boxes for the same
 * keys, most of them small.  verdicts[i] and digests32[32 i .. 32 i + 31] (optional) are what
 * mpvss_modp_group_verify_distribution -- for a box with a key set, mpvss_modp_group_verify_distribution_keyset -- gives for
 * boxes[i] on the same context, byte for byte, at every width and under every mode of mpvss_ctx_set_rt_fd; a box with n == 0
 * hashes the empty transcript.  Runs of consecutive small boxes (1 <= n, t <= 16384) that take their keys the same way -- all
 * from arrays, or all from one and the same key set -- travel through the GPU as one batch of at most MPVSS_MAX_CHUNK shares;
 * every other box, and a run of one, takes the one-box path.
 * The array pointers of a box live in `space`; challenge_host, boxes, verdicts and digests32 are host memory; keyset != NULL:
 * pubkeys is ignored and may be NULL.  The call is synchronous, holds the context lock like its one-box sibling and has no
 * dumps of X, a1, a2.  hash_threads: up to that many host threads hash the transcripts of a run's boxes (clamped to 1..16;
 * <= 0: the library chooses, at most 16).
 * ERRORS: count == 0 is MPVSS_OK; no context or no group, and boxes or verdicts NULL with count > 0, are MPVSS_E_INVALID.  A
 * malformed box -- a required pointer NULL (with n > 0; the challenge always), t == 0 with n > 0, n or t above 0x7fffffff, a key
 * set of another context or another modulus, key_offset + n beyond the set -- costs only itself: verdict 0, a digest of zeros,
 * and the call goes on and returns MPVSS_OK (as mpvss_modp_verify_many).  A negative position, a HIP error or a failed
 * allocation ends the call with the code the one-box call returns and leaves the context usable.
 * mpvss_modp_group_verify_many_stats: since the context was created, the grouped passes, the boxes that went through them and
 * the boxes that went through the one-box path (empty and malformed boxes are in neither); any pointer may be NULL. */
typedef struct mpvss_modp_group_box {
  const uint8_t* commitments; size_t t;
  const int64_t* positions;
  const uint8_t* pubkeys; const uint8_t* shares; const uint8_t* responses; size_t n;
  const uint8_t* challenge_host;
  const mpvss_modp_group_keyset* keyset; size_t key_offset;
} mpvss_modp_group_box;
int mpvss_modp_group_verify_many(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_box* boxes, size_t count,
                                 int hash_threads, int* verdicts, uint8_t* digests32);
int mpvss_modp_group_verify_many_stats(mpvss_ctx* ctx, unsigned long long* groups, unsigned long long* grouped_boxes,
                                       unsigned long long* single_boxes);

/* Many secrets in one call.  After verifying, a participant of a round reconstructs one secret per dealer, usually from the same
 * responding participants.  For every secret i that mpvss_modp_group_reconstruct accepts, status[i] == MPVSS_OK and
 * gs_out[i eb .. i eb + eb - 1] (eb = mpvss_modp_group_elem_bytes) and masks_out32[32 i .. 32 i + 31] (optional) are what that
 * call gives for (positions_host, shares, m) on the same context, byte for byte, at every width and in both spaces; in device
 * space the share buffers are left unchanged.  The Lagrange coefficients are computed once per distinct position list of the call
 * (lists are equal when their sequences are: a permuted list is another list).  Runs of consecutive secrets of at most 16384
 * shares each travel through the GPU as one batch of at most MPVSS_MAX_CHUNK shares, one workgroup per secret for the product;
 * every longer secret, and a run of one, takes the one-secret path.
 * shares live in `space`; positions_host, secrets, status, gs_out and masks_out32 are host memory.  The call is synchronous and
 * holds the context lock like its one-secret sibling.  host_threads: up to that many host threads compute the Lagrange
 * coefficients and the masks (clamped to 1..16; <= 0: the library chooses from the work of the call, at most 16, never by the
 * machine's CPU count).
 * ERRORS: count == 0 is MPVSS_OK; no context or no group, and secrets, status or gs_out NULL with count > 0, are MPVSS_E_INVALID
 * and write no output.  A refused secret -- whatever the one-secret call answers with MPVSS_E_INVALID: a pointer NULL, m == 0,
 * m above 0x7fffffff, a position below 1, duplicate positions, a coefficient whose reduced denominator has no inverse mod
 * (q-1)/2, an even (q-1)/2, a share that is 0 mod q under a negative coefficient -- costs only itself: that code in status[i],
 * zeros in gs_out[i] and in its mask, and the call goes on and returns MPVSS_OK.  A HIP error or a failed allocation ends the call
 * with the code the one-secret call returns and leaves the context usable.
 * mpvss_modp_group_reconstruct_many_stats: since the context was created, the grouped passes, the secrets that went through them
 * and the secrets that took the one-secret path (refused secrets are in none); any pointer may be NULL, no context is
 * MPVSS_E_INVALID. */
typedef struct mpvss_modp_group_secret {
  const int64_t* positions_host;   /* m positions, host memory in either space */
  const uint8_t* shares;           /* m x element size, in `space` */
  size_t m;
} mpvss_modp_group_secret;
int mpvss_modp_group_reconstruct_many(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const mpvss_modp_group_secret* secrets,
                                      size_t count, int host_threads, int* status, uint8_t* gs_out, uint8_t* masks_out32);
int mpvss_modp_group_reconstruct_many_stats(mpvss_ctx* ctx, unsigned long long* passes, unsigned long long* grouped_secrets,
                                            unsigned long long* single_secrets);

/* Where mpvss_modp_group_reconstruct and mpvss_modp_group_reconstruct_many compute the Lagrange exponents of a position list,
 * |lambda_i| = prod_{j != i} x_j / |x_j - x_i| mod (q-1)/2 written as the exponent of share i (participant.rs:526-561): mode 0 on
 * the host as before; 2 on the device whenever the list is admitted -- the handle has the device scalar ring
 * (mpvss_modp_group_has_device_scalar), no list of more than 16384 positions, fewer than 2^31 positions in all --; 1, the
 * default, on the device when the work of the call (the sum of m^2 over its distinct lists; m^2 of a lone secret) reaches a
 * measured size: 60 x 32^2 = 61 440 up to 2048 bits, 60 x 1024^2 at the 384- and 512-byte handles ("Lagrange
 * exponents on the device"; profiles/modp_rt_lagrange_device.txt).  On the device k_rt_lagrange_terms forms numerator and denominator
 * of every coefficient (one DPP quad each, a tile of up to 16 coefficients of one list per workgroup), the denominators are
 * inverted by Fermat's power through the group's own table and exponentiation kernels, and k_rt_lagrange_finish checks
 * den * den^-1 = 1 and stores the exponent; a list with a failed check -- a denominator that is 0 mod a small (q-1)/2, a composite
 * (q-1)/2 -- is computed again, whole, by the host path, which decides between a value (the fraction in lowest terms) and a
 * refusal.  Every exponent is the host's byte for byte, so the results of all reconstruct entry points are the same bytes under
 * every mode.  Returns the mode before; no context, or another value, is MPVSS_E_INVALID. */
int mpvss_ctx_set_rt_lagrange(mpvss_ctx* ctx, int mode);
/* The exponents on their own: exps_out_host[i eb .. i eb + eb - 1] (eb = mpvss_modp_group_elem_bytes, big-endian) = the exponent
 * share i of a secret at these positions is raised to: |lambda_i| mod (q-1)/2, or (q-1) - |lambda_i| for a negative coefficient
 * of nonzero magnitude; computed where the context's mode says.  Refusals are those of mpvss_modp_group_reconstruct: a NULL pointer,
 * m == 0, m above 0x7fffffff, a position below 1, duplicate positions, a coefficient whose reduced denominator has no inverse mod
 * (q-1)/2 are MPVSS_E_INVALID and leave the output untouched.  Synchronous, under the context lock. */
int mpvss_modp_group_lagrange_exponents(mpvss_ctx* ctx, const mpvss_modp_group* grp, const int64_t* positions_host, size_t m,
                                        uint8_t* exps_out_host);
/* Position lists whose exponents were computed on the device / on the host since the context was created, by any of the three
 * calls above, and fallback_lists, the lists tried on the device and done again on the host (they are counted in host_lists too,
 * not in device_lists).  A list shared by several secrets of one call counts once; refused lists are in none of the counts.  Any
 * pointer may be NULL; no context is MPVSS_E_INVALID. */
int mpvss_modp_group_lagrange_stats(mpvss_ctx* ctx, unsigned long long* device_lists, unsigned long long* host_lists,
                                    unsigned long long* fallback_lists);

/* The row layout for small calls of a run-time group.  The quad layout (4 lanes per number, 16 numbers per wave) is sized for a
 * full chip; a call of a handful to a few thousand numbers is the latency of ONE number's chain of 2 000 to 5 000 Montgomery
 * operations.  On the row layout (16 lanes per number, 4 numbers per wave; 5 / 7 / 9 limbs per lane instead of 18 / 27 / 36) about a third
 * of the instructions lie on that chain.  It exists for the handles at 18, 27 and 36 limbs per lane (moduli of 1043 .. 4096 bits) and
 * for the launches of k_rt_dual_exp, k_rt_exp_sets and k_rt_comb_exp: every mpvss_modp_group_* call that reaches one of them --
 * batch_exp, batch_exp_fixed_base, the small path of batch_twin_exp, dleq_commitments, verify_distribution, verify_shares, deal,
 * distribute, extract_shares, reconstruct, the Lagrange inverses, and the grouped runs of verify_many / reconstruct_many by their total
 * share count.  Results are the same bytes under every mode.
 * mode 0 = never (the default); 1 = automatic: launches of at most mpvss_modp_group_row_max_shares numbers; 2 = whenever the handle
 * has the layout, at any count.  Returns the mode before; no context, or another value, is MPVSS_E_INVALID.
 * Not on the row layout: the key-set kernels, X_i (commit_eval, forward differences), the shared-squarings twin kernel, handles at 5 /
 * 9 limbs per lane, the pair / MFMA layout; the run-time calls stay on one stream ("Row layout for small calls"). */
int mpvss_ctx_set_rt_row(mpvss_ctx* ctx, int mode);
/* Numbers of one launch up to which mode 1 takes the row layout: 4096 -- four numbers per wave on 1 024 SIMDs, one wave per SIMD, the
 * derivation group 14 uses, not a measurement -- or 0 for a handle at 5 or 9 limbs per lane and for no group. */
int mpvss_modp_group_row_max_shares(const mpvss_modp_group* grp);
/* Launches through the three routed sites since the context was created, by the layout they took.  Either pointer may be NULL; no
 * context is MPVSS_E_INVALID. */
int mpvss_modp_group_row_stats(mpvss_ctx* ctx, unsigned long long* row_launches, unsigned long long* quad_launches);

/* ---- hashing helpers (host only; Group::hash_to_scalar, src/groups/modp.rs:142-148) ------ */

/* out32 = SHA-256(data) */
void mpvss_sha256(const uint8_t* data, size_t len, uint8_t out32[32]);
/* out256 = int_BE(SHA256(data)) mod (q-1)/2 as 256-byte big-endian */
void mpvss_modp_hash_to_scalar(const uint8_t* data, size_t len, uint8_t out256[256]);

/* ---- timing hooks for bench.py ------------------------------------------------------------ */

/* Milliseconds the GPU spent in the kernels of the most recent compute call on this context,
 * measured with hipEvents on the stream each kernel was launched on, summed per kind:
 *   0 = the X path (k_modp_commit_eval and, for consecutive positions, the forward-difference kernels),
 *   1 = k_modp_comb_dual_exp (a1), 2 = table builds, 3 = k_modp_dual_exp (a2, batch_exp),
 *   4 = the scalar-ring kernels of a run-time group (k_rt_modq_*), the launches of its Lagrange exponents (k_rt_lagrange_terms, the
 *       denominators' tables and powers, k_rt_lagrange_finish), and k_ec_lagrange of the curve groups.
 * Kernels of different kinds may overlap in time (two streams), so the sums can exceed the wall time.
 * mpvss_last_kernel_launches gives the number of launches behind each sum.  Negative when unavailable. */
double mpvss_last_kernel_ms(const mpvss_ctx* ctx, int kernel_id);
int mpvss_last_kernel_launches(const mpvss_ctx* ctx, int kernel_id);
/* Absorbed verify blocks whose X_i went through the forward-difference path, and how many of those fell back to
 * Horner's rule on the device (positions not consecutive, an X that is 0 mod q, a pipeline stage that gave up):
 * same results either way, the fall-back is just slower -- a counter for operators and tests.  The curve groups' blocks whose
 * X path ran behind a device gate (stage pipelines, device-resident positions) count the same way. */
int mpvss_modp_fd_stats(mpvss_ctx* ctx, unsigned long long* blocks, unsigned long long* fallbacks);

/* Host-side accounting of the block pipeline (verify_block_compute / _absorb / verify_many), sums over the blocks
 * absorbed since the last reset: time the calling threads spent enqueueing GPU work, waiting for the GPU and
 * hashing transcripts, and the per-kind kernel durations of mpvss_last_kernel_ms summed over those blocks. */
typedef struct mpvss_pipeline_stats {
  double enqueue_ms, wait_ms, hash_ms;
  double kernel_ms[4];
  unsigned long long kernel_launches[4];
  unsigned long long blocks;
} mpvss_pipeline_stats;
int mpvss_pipeline_stats_get(mpvss_ctx* ctx, mpvss_pipeline_stats* out, int reset);
/* Blocks of the block API currently in flight in this context (enqueued, not yet fully absorbed) and how many of them
 * still have GPU work pending: for monitoring and for callers that schedule compute / absorb themselves. */
int mpvss_blocks_in_flight(mpvss_ctx* ctx, int* in_flight_out, int* gpu_pending_out);
/* 1 when the transcript hash uses the CPU's SHA extensions (about 1.7 GB/s per thread), 0 for the portable code */
int mpvss_sha256_uses_shani(void);
/* Measurement aid (no reference counterpart): what this device sustains, now, of the instruction the kernels are made of -- four
 * waves per SIMD on every CU issue it back to back for about target_ms.  kind 0: v_mad_u64_u32 (the limb product of all three
 * groups), kind 1: 32-bit integer work (v_add3_u32, v_and_b32, v_lshl_add_u32), 2: the 64-bit shifts of a retire step (v_lshl_add_u64,
 * v_lshrrev_b64), 3: v_permlane32_swap, 4: v_mov_b64, 5: VOP2 v_add_u32 -- the classes bench.py prices the kernels' instruction mix
 * with (`compute.peak_mix_weighted`).  Wave-instructions per second over the whole chip, the shader clock the waves saw
 * (s_memtime against the 100 MHz s_memrealtime) and the duration; the last two are optional. */
int mpvss_issue_probe(mpvss_ctx* ctx, int kind, double target_ms, double* insts_per_s_out, double* shader_clock_ghz_out,
                      double* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* MPVSS_HIP_H */
