// The plan of the X path of the fixed 2048-bit group (eval_x in mpvss_capi.cpp): which kernels compute X_i for a run of shares, with
// what geometry, and how much workspace they need.  Every host-side decision of that path is taken here, once per chunk, from values
// the caller has read once; eval_x only ensures the buffers and enqueues what the plan says.  Plain C++: no HIP, no context, no
// getenv, so that tests/test_fd_plan_host.py runs the very code the library runs (tests/fd_plan_shim.cpp), on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "modp_limbs.h"

namespace fdplan {

constexpr size_t ROW_MAX_NUMBERS = 4096;           // up to here a lone batch takes the row layout (one wave per SIMD)
constexpr size_t NUMBER_BYTES = limbs::L * 4;      // a number in Montgomery limbs

// the environment's say, read once per process by the library
struct Knobs {
  int fd = 1;                  // MPVSS_FD: 0 disables the path (every X by the Horner kernel)
  size_t min_shares = 4096;    // MPVSS_FD_MIN_SHARES: the batch size the path is used from (tests lower it)
  size_t pair_min_t = 512;     // MPVSS_FD_PAIR_MIN_T: the pair-layout stepping from this many commitments ...
  bool pair_step = true;       // ... when MPVSS_PAIR bit 5 is set
  int tile = 0;                // MPVSS_FD_TILE (with the pair-layout stepping): 0 never, 1 when other blocks are in flight, 2 always
  int tile_steps = 64;         // MPVSS_FD_TILE_STEPS
  int l1 = 1;                  // MPVSS_FD_L1, two-level seeding: 0 never, 1 when other blocks are in flight, 2 always
  int test_fault = 0;          // MPVSS_FD_TEST_FAULT (tests only): 1 / 2 a stage of the stepping pipelines gives up, 3 of the
                               // stride-1 seeding chain, 4 of the table pipeline
};

// are the n positions consecutive from a start in [0, 2^61)?  (what the forward differences of either group family step through;
// n == 0: no)
inline bool positions_consecutive(const int64_t* hpos, size_t n) {
  if (n == 0 || hpos[0] < 0 || hpos[0] >= ((int64_t)1 << 61)) return false;
  for (size_t i = 1; i < n; ++i)
    if (hpos[i] != hpos[0] + (int64_t)i) return false;
  return true;
}

// does the forward-difference path apply to this run of shares?  The host-side part of the decision: host positions are judged
// here, device positions (hpos == nullptr) by a kernel that clears the path's flag.
inline bool applies(const Knobs& k, size_t t, size_t cnt, const int64_t* hpos) {
  constexpr size_t max_t = 1024;
  const bool fd = k.fd && t >= 16 && t <= max_t && cnt >= 16 * t && cnt >= k.min_shares;
  return fd && (hpos == nullptr || positions_consecutive(hpos, cnt));
}

enum Path { HORNER_ROW, HORNER, FORWARD_DIFFERENCES };
enum Seeds { SEEDS_NONE, SEEDS_ROW, SEEDS_QUAD };          // the Horner kernel of a seeding level (none: the level is not Horner's)
enum Step { STEP_QUAD, STEP_PAIR, STEP_PAIR_TILED };

// Chain c of S owns the positions c, c+S, c+2S, .. (index j inside the chain); its seeds are the t indices w0 .. w0+t-1 in the
// MIDDLE of the chain, from which one pipeline steps forward and one backward: the seeds of all chains together are the m0 = S t
// consecutive positions from seed0 = S w0.  Level 2 is those chains.  Level 1 (two_level) is one chain of stride 1 over the seed
// window, from Horner's rule at the t positions w1 .. w1+t-1 in ITS middle.
struct Plan {
  size_t t = 0, cnt = 0, boxes = 1;      // what was asked for
  bool busy = false, x_alone = false;
  Path path = HORNER;
  bool fd = false;                       // path == FORWARD_DIFFERENCES; everything below is set on that path only
  bool device_positions = false;         // nobody has looked at the positions yet: a kernel checks them
  size_t S = 0, chain_len = 0, w0 = 0, seed0 = 0, m0 = 0, w1 = 0;
  bool two_level = false;
  Seeds seeds1 = SEEDS_NONE, seeds2 = SEEDS_NONE;
  Step step1 = STEP_QUAD, step2 = STEP_QUAD;
  int fault_table1 = 0, fault_step1 = 0, fault_table2 = 0, fault_step2 = 0;    // what each pipeline launch is handed
  int tile_steps = 64;
};

// the forward-difference fields of p from its t, cnt, busy and x_alone
inline void lay_chains(const Knobs& k, Plan& p) {
  const size_t t = p.t, cnt = p.cnt;
  // The seed launch is latency-bound (2048 seeds are an eighth of a wave per SIMD), so fewer seeds would not finish sooner; more
  // chains shorten the stepping but cost Horner work.  Measured optima on MI355X: chains of about 8192 members, fewer when the
  // seeds are dear (t = 512: 4), never longer than 16384 members (n=131072, t=1024: 8)
  size_t S = std::max<size_t>(std::max<size_t>(std::min<size_t>(2048 / t, cnt / 8192), cnt / 16384), 4);
  // A call that has the GPU to itself: more, shorter chains -- the extra seeds are one wide launch on an idle chip, the stepping
  // (the serial part) shrinks in proportion.
  // ... and a box among others of at least 65536 shares: its X path is a chain of dependent launches that holds one hardware queue
  // from its first kernel to a1, and the boxes in flight share GPU_MAX_HW_QUEUES of them, so a box cannot come sooner than its
  // chain's span over the queues (profiles/x_chain_trace_parent.txt: 4 queues, 4 X paths open, 207 ms / 3.4 = 61 ms per box).
  // With the stride-1 seeding chain stepping both ways 16 chains are 2 175 + 2 175 serial steps instead of 8 chains'
  // 1 151 + 4 223, for about 25 products per share more (profiles/x_chain_ab.txt).
  constexpr size_t lone_chains = 16;     // measured: 8 -> 109 ms per box, 16 -> 96.5, 32 -> 104, 64 -> 115
  if (lone_chains > S && (!p.busy || cnt >= 65536) && t <= 256) S = lone_chains;
  S = std::max<size_t>(std::min(S, cnt / (4 * t)), 1);      // (cnt >= 16 t where the path applies, so at least 4)
  p.S = S;
  p.chain_len = (cnt + S - 1) / S;
  p.w0 = (p.chain_len - t) / 2;                             // (S <= cnt / 4t: a chain has at least 4 t members)
  p.seed0 = S * p.w0;
  p.m0 = S * t;
  // Two-level seeding: Horner's rule -- about 7 000 products per seed at (65536, 256) -- only for the middle t of the S t seed
  // positions; the stride-1 chain steps through the remaining (S-1) t at t products each, forward and backward at once:
  // max(m0 - 1 - w1, w1 + t - 1) serial steps instead of m0 - 1.  Same values (uniqueness of the group element); 180 products per
  // share fewer at (65536, 256), for about 15 ms more latency of the box's chain: a call that has the GPU to itself keeps the wide
  // Horner launch for all S t seeds.  m0 == t never gets there (S > 1), and w1 == 0 would be forward only.
  p.two_level = S > 1 && (k.l1 >= 2 || (k.l1 == 1 && p.busy));
  p.w1 = (p.m0 - t) / 2;
  // The t first-level seeds are 16 waves of the quad layout whose latency is the whole cost (about 5 600 dependent operations): the
  // row layout does an operation in 3.5 instead of 5.7 us, and its 1.3x issue slots on t seeds are 0.4 % of the box.  All S t seeds
  // take the row layout only where nothing of the caller runs beside this X path (x_alone) and the chip is the call's own.
  p.seeds1 = p.two_level ? SEEDS_ROW : SEEDS_NONE;
  p.seeds2 = p.two_level ? SEEDS_NONE : (p.x_alone && !p.busy) ? SEEDS_ROW : SEEDS_QUAD;
  p.fault_table2 = p.fault_step2 = k.test_fault;
  p.fault_table1 = 0;
  p.fault_step1 = k.test_fault == 3 ? 1 : 0;
  // The stepping kernels on the pair layout from pair_min_t commitments: stages of 32 levels, 122 instead of 191 issue slots per
  // product, but half as many waves with longer steps (profiles/r03_fd_pair_ab.txt).  Tiled: the stepping as wide launches over the
  // anti-diagonals of the (stage, block of tile_steps steps) grid instead of a pipeline of persistent stages -- no wave waits for
  // another one, and none can be told to give up (a lone call keeps the pipeline under tile == 1: its latency is shorter).
  const bool pair = k.pair_step && t >= k.pair_min_t;
  const bool tiled = pair && (k.tile >= 2 || (k.tile == 1 && p.busy));
  auto step_of = [&](int fault) { return tiled && fault == 0 ? STEP_PAIR_TILED : pair ? STEP_PAIR : STEP_QUAD; };
  p.step1 = step_of(p.fault_step1);
  p.step2 = step_of(p.fault_step2);
  p.tile_steps = k.tile_steps;
}

// THE decision of the X path for `boxes` same-shaped boxes of cnt shares and t commitments each.
//   busy     other blocks are in flight on the context (read once by the caller)
//   x_alone  nothing of the caller runs beside this X path
//   direct   Horner for every share whatever the positions are
//   hpos     the positions where the host has them (nullptr: device-resident)
inline Plan plan(const Knobs& k, size_t t, size_t cnt, size_t boxes, bool busy, bool x_alone, bool direct, const int64_t* hpos) {
  Plan p;
  p.t = t;
  p.cnt = cnt;
  p.boxes = boxes;
  p.busy = busy;
  p.x_alone = x_alone;
  if (direct || !applies(k, t, cnt, hpos)) {
    // a small lone box is the latency of one share's Horner chain ((t - 1) x about 26 operations): the row layout's kernel, 3.5
    // instead of 5.7 us per operation
    p.path = boxes == 1 && cnt <= ROW_MAX_NUMBERS ? HORNER_ROW : HORNER;
    return p;
  }
  p.path = FORWARD_DIFFERENCES;
  p.fd = true;
  p.device_positions = hpos == nullptr;
  lay_chains(k, p);
  return p;
}

// Product tree of the simultaneous inversion of m numbers: level l turns ms[l] numbers into ms[l+1] totals of G of them, down to
// one root.  The prefix products of level l < levels() start at number pre_off[l] of fd_pre, the totals (and their inverses) of
// level l >= 1 at number tot_off[l] of fd_tot (fd_totinv); `pre` and `tot` numbers in all.
struct InvTree {
  static constexpr size_t G = 16;
  std::vector<size_t> ms, pre_off, tot_off;
  size_t pre = 0, tot = 0;
  size_t levels() const { return ms.size() - 1; }
};

inline InvTree tree(size_t m) {
  InvTree tr;
  tr.ms.push_back(m);
  while (tr.ms.back() > 1) tr.ms.push_back((tr.ms.back() + InvTree::G - 1) / InvTree::G);
  const size_t nlev = tr.levels();
  tr.pre_off.assign(nlev + 1, 0);
  tr.tot_off.assign(nlev + 1, 0);
  for (size_t l = 0; l < nlev; ++l) { tr.pre_off[l] = tr.pre; tr.pre += tr.ms[l]; }
  for (size_t l = 1; l <= nlev; ++l) { tr.tot_off[l] = tr.tot; tr.tot += tr.ms[l]; }
  return tr;
}

// What one plan needs, in bytes, of the workspace's fd_* buffers (fd_totinv: as fd_tot), and where a box's parts lie in the two
// hand-over buffers of the pipelined kernels: box b's words start at b * box_hand_t (box_hand_s) bytes, level 2's first, level 1's
// from hand_t1_off (hand_s1_off) -- [tables L2][stepping L2][tables L1][stepping L1] per box over the two buffers.
struct Bytes {
  size_t xm = 0, xinv = 0, pre = 0, tot = 0, state = 0, gather = 0, hand_t = 0, hand_s = 0;
  size_t box_hand_t = 0, box_hand_s = 0, hand_t1_off = 0, hand_s1_off = 0;
};

// table_words(chains, t) and step_words(chains, t, chain_len): 32-bit words of hand-over buffer a table / stepping launch needs
// (constants of the kernels' translation unit: modp_fd_table_hand_words, modp_fd_step_hand_words)
template <class TableWords, class StepWords>
Bytes bytes(const Plan& p, TableWords table_words, StepWords step_words) {
  Bytes b;
  if (!p.fd) return b;
  const InvTree tr = tree(p.boxes * p.m0);       // the larger of the two inversions: all seeds of all boxes side by side
  b.xm = p.boxes * p.cnt * NUMBER_BYTES;
  b.xinv = p.boxes * p.m0 * NUMBER_BYTES;
  b.pre = tr.pre * NUMBER_BYTES;
  b.tot = tr.tot * NUMBER_BYTES;
  b.state = p.boxes * 2 * p.m0 * NUMBER_BYTES;
  b.gather = p.boxes > 1 ? b.xinv : 0;
  b.hand_t1_off = (size_t)table_words(p.S, p.t) * 4;
  b.hand_s1_off = (size_t)step_words(p.S, p.t, p.chain_len) * 4;
  b.box_hand_t = b.hand_t1_off + (p.two_level ? (size_t)table_words((size_t)1, p.t) * 4 : 0);
  b.box_hand_s = b.hand_s1_off + (p.two_level ? (size_t)step_words((size_t)1, p.t, p.m0) * 4 : 0);
  b.hand_t = p.boxes * b.box_hand_t;
  b.hand_s = p.boxes * b.box_hand_s;
  return b;
}

// What the workspace is grown to for plan p: the chains and seeding levels depend on whether other blocks are in flight, and a slot
// sees both over its life, so the buffers take the larger of the two plans at once -- growing one later means hipFree, which waits
// for the device (58-87 ms inside the enqueue of a timed box, measured with MPVSS_TRACE_ENQUEUE).  The layout fields are p's own.
template <class TableWords, class StepWords>
Bytes sized(const Knobs& k, const Plan& p, TableWords table_words, StepWords step_words) {
  Bytes b = bytes(p, table_words, step_words);
  if (!p.fd) return b;
  Plan other = p;
  other.busy = !p.busy;
  lay_chains(k, other);
  const Bytes o = bytes(other, table_words, step_words);
  size_t Bytes::*const buffers[] = {&Bytes::xm,    &Bytes::xinv,   &Bytes::pre,    &Bytes::tot,
                                    &Bytes::state, &Bytes::gather, &Bytes::hand_t, &Bytes::hand_s};
  for (auto f : buffers) b.*f = std::max(b.*f, o.*f);
  return b;
}

}  // namespace fdplan
