// The plan of the fixed group's X path (mpvss_rs_amd/csrc/host_fd_plan.h) compiled for the CPU, for tests/test_fd_plan_host.py:
// the very decisions, geometry, inversion tree and workspace sizes the library computes.  Test infrastructure, never shipped.
// The hand-over word counts belong to the kernels' translation unit; here they are stand-ins: table(ch, t) = 7 ch t,
// step(ch, t, len) = 3 ch (len + t).
// With -DFD_PLAN_MAIN the file is a stand-alone program that walks the test's grid and cnt = 2^31 - 1 (a sanitizer build of it runs
// on its own, outside Python).
#include <stdint.h>

#include "../mpvss_rs_amd/csrc/host_fd_plan.h"

namespace {

size_t table_words(size_t chains, size_t t) { return 7 * chains * t; }
size_t step_words(size_t chains, size_t t, size_t len) { return 3 * chains * (len + t); }

// knobs as eight numbers: MPVSS_FD, _MIN_SHARES, _PAIR_MIN_T, bit 5 of the pair mask, _TILE, _TILE_STEPS, _L1, _TEST_FAULT
fdplan::Knobs knobs_of(const int64_t* k) {
  fdplan::Knobs kn;
  kn.fd = (int)k[0];
  kn.min_shares = (size_t)k[1];
  kn.pair_min_t = (size_t)k[2];
  kn.pair_step = k[3] != 0;
  kn.tile = (int)k[4];
  kn.tile_steps = (int)k[5];
  kn.l1 = (int)k[6];
  kn.test_fault = (int)k[7];
  return kn;
}

void put_bytes(const fdplan::Bytes& b, int64_t* out) {
  const size_t v[12] = {b.xm, b.xinv, b.pre, b.tot, b.state, b.gather, b.hand_t, b.hand_s, b.box_hand_t, b.box_hand_s, b.hand_t1_off,
                        b.hand_s1_off};
  for (int i = 0; i < 12; ++i) out[i] = (int64_t)v[i];
}

}  // namespace

extern "C" {

int fd_applies_c(const int64_t* knobs, size_t t, size_t cnt, const int64_t* hpos) { return fdplan::applies(knobs_of(knobs), t, cnt, hpos); }

// out[19]: path, fd, device_positions, S, chain_len, w0, seed0, m0, w1, two_level, seeds1, seeds2, step1, step2, fault_table1,
// fault_step1, fault_table2, fault_step2, tile_steps.  bytes[12], sized[12]: the plan's own Bytes and what the workspace is grown
// to -- xm, xinv, pre, tot, state, gather, hand_t, hand_s, box_hand_t, box_hand_s, hand_t1_off, hand_s1_off.
void fd_plan_c(const int64_t* knobs, size_t t, size_t cnt, size_t boxes, int busy, int x_alone, int direct, const int64_t* hpos,
               int64_t* out, int64_t* bytes, int64_t* sized) {
  const fdplan::Knobs k = knobs_of(knobs);
  const fdplan::Plan p = fdplan::plan(k, t, cnt, boxes, busy != 0, x_alone != 0, direct != 0, hpos);
  const int64_t v[19] = {p.path,   p.fd,      p.device_positions, (int64_t)p.S, (int64_t)p.chain_len, (int64_t)p.w0,  (int64_t)p.seed0,
                         (int64_t)p.m0, (int64_t)p.w1, p.two_level,   p.seeds1,     p.seeds2,             p.step1,        p.step2,
                         p.fault_table1, p.fault_step1, p.fault_table2, p.fault_step2, p.tile_steps};
  for (int i = 0; i < 19; ++i) out[i] = v[i];
  put_bytes(fdplan::bytes(p, table_words, step_words), bytes);
  put_bytes(fdplan::sized(k, p, table_words, step_words), sized);
}

// the inversion tree of m numbers: ms[0 .. levels], pre_off[0 .. levels), tot_off[1 .. levels] (entry 0 is 0), totals = {pre, tot};
// returns the number of levels, -1 when the arrays (cap entries each) are too short
long fd_tree_c(size_t m, int64_t* ms, int64_t* pre_off, int64_t* tot_off, size_t cap, int64_t* totals) {
  const fdplan::InvTree tr = fdplan::tree(m);
  if (tr.ms.size() > cap) return -1;
  for (size_t l = 0; l < tr.ms.size(); ++l) {
    ms[l] = (int64_t)tr.ms[l];
    pre_off[l] = (int64_t)tr.pre_off[l];
    tot_off[l] = (int64_t)tr.tot_off[l];
  }
  totals[0] = (int64_t)tr.pre;
  totals[1] = (int64_t)tr.tot;
  return (long)tr.levels();
}
}

#ifdef FD_PLAN_MAIN
#include <stdio.h>

int main() {
  long bad = 0, plans = 0;
  const size_t ts[] = {16, 17, 31, 32, 64, 255, 256, 257, 511, 512, 1024};
  for (size_t t : ts) {
    const size_t cnts[] = {16 * t, 16 * t + 1, 4095, 4096, 8192, 16384, 65535, 65536, 131072, ((size_t)1 << 31) - 1};
    for (size_t cnt : cnts)
      for (size_t boxes = 1; boxes <= 3; ++boxes)
        for (int busy = 0; busy < 2; ++busy)
          for (int64_t l1 = 0; l1 < 3; ++l1)
            for (int64_t fault = 0; fault < 5; fault += 3) {
              const int64_t knobs[8] = {1, 256, 512, 1, busy, 37, l1, fault};
              int64_t p[19], own[12], sized[12];
              fd_plan_c(knobs, t, cnt, boxes, busy, boxes == 1, 0, nullptr, p, own, sized);
              ++plans;
              if (cnt < 16 * t) {          // not admissible: Horner, and nothing laid out
                bad += p[1] != 0 || p[3] != 0;
                continue;
              }
              const int64_t S = p[3], chain_len = p[4], w0 = p[5], seed0 = p[6], m0 = p[7], w1 = p[8];
              bad += p[1] != 1 || S < 1 || w0 < 0 || seed0 + m0 > (int64_t)cnt || S * chain_len < (int64_t)cnt;
              bad += p[9] && !(S > 1 && 0 < w1 && w1 + (int64_t)t <= m0);
              for (int i = 0; i < 8; ++i) bad += sized[i] < own[i];
              int64_t ms[16], pre_off[16], tot_off[16], totals[2];
              const long nlev = fd_tree_c(boxes * (size_t)m0, ms, pre_off, tot_off, 16, totals);
              bad += nlev < 1 || ms[0] != (int64_t)boxes * m0 || ms[nlev] != 1;
              bad += totals[0] * (int64_t)fdplan::NUMBER_BYTES != own[2] || totals[1] * (int64_t)fdplan::NUMBER_BYTES != own[3];
            }
  }
  // positions: a gap, a negative start, starts at the end of the admitted range
  const int64_t knobs[8] = {1, 256, 512, 1, 0, 64, 1, 0};
  int64_t pos[256];
  for (int64_t start : {(int64_t)0, (int64_t)-1, ((int64_t)1 << 61) - 1, (int64_t)1 << 61}) {
    for (int i = 0; i < 256; ++i) pos[i] = start + i;
    bad += fd_applies_c(knobs, 16, 256, pos) != (start >= 0 && start < ((int64_t)1 << 61));
  }
  for (int i = 0; i < 256; ++i) pos[i] = 5 + i + (i == 255);
  bad += fd_applies_c(knobs, 16, 256, pos) != 0;
  printf(bad ? "fd_plan_shim: %ld checks failed\n" : "fd_plan_shim: ok (%ld plans)\n", bad ? bad : plans);
  return bad ? 1 : 0;
}
#endif
