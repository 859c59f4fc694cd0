// The host side that the *_many entry points share (mpvss_rs_amd/csrc/host_many.h) compiled for the CPU, for
// tests/test_many_host.py: the very walk, plan and tile table the library runs.  Test infrastructure, never shipped.
// With -DMANY_HOST_MAIN the file is a stand-alone program that drives the same functions once (a sanitizer build of it runs on
// its own, outside Python).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../mpvss_rs_amd/csrc/host_many.h"

namespace {

struct Secret {             // the three members of mpvss_modp_group_secret and mpvss_ec_secret
  const int64_t* positions_host;
  const uint8_t* shares;
  size_t m;
};

}  // namespace

extern "C" {

int many_threads_c(int requested, size_t work, size_t per_thread) { return many::many_threads(requested, work, per_thread); }

// The walk over count items of kinds[] (many::Kind), costs a[] and b[]; an item joins a run when its key equals the key of the
// run's first item.  Every call of alone or pass appends an event to events[]: {0, i} or {len, i0, i1, ...}.  The fail_at-th call
// (0-based; -1: none) returns fail_code.  Returns the walk's code; *n_words: words written (-1: events[] was too short).
int many_walk_c(size_t count, const int* kinds, const size_t* a, const size_t* b, const int64_t* keys, size_t cap_a, size_t cap_b,
                long fail_at, int fail_code, int64_t* events, size_t events_cap, long* n_words) {
  size_t at = 0;
  long calls = 0;
  bool overflow = false;
  auto put = [&](int64_t v) {
    if (at < events_cap) events[at++] = v;
    else overflow = true;
  };
  const int rc = many::walk(
      count, cap_a, cap_b, [&](size_t i) { return (many::Kind)kinds[i]; }, [&](size_t i) { return many::Cost{a[i], b[i]}; },
      [&](size_t first, size_t i) { return keys[first] == keys[i]; },
      [&](size_t i) {
        put(0);
        put((int64_t)i);
        return calls++ == fail_at ? fail_code : 0;
      },
      [&](const std::vector<size_t>& run) {
        put((int64_t)run.size());
        for (size_t i : run) put((int64_t)i);
        return calls++ == fail_at ? fail_code : 0;
      });
  *n_words = overflow ? -1 : (long)at;
  return rc;
}

// The plan over count secrets: secret i has m[i] positions at pos + pos_off[i] (pos_off[i] < 0: a null pointer) and shares or
// none.  The coefficient function counts its visits of every slot c in visits[c] and notes what it was asked for: the list's
// length in seen_m[c], the index in seen_j[c], the position at that index in seen_pos[c]; it fails where that position equals
// fail_pos.  The three arrays hold slots_cap entries; returns -1 when the plan needs more, else the number of distinct lists.
long many_plan_c(size_t count, const int64_t* pos, const long* pos_off, const size_t* m, const int* has_shares, size_t cap_each,
                 size_t cap_run, int host_threads, int64_t fail_pos, int* kind, size_t* coef, size_t* list_of, size_t* list_first,
                 size_t* list_m, size_t* coefs, size_t slots_cap, int* visits, size_t* seen_m, size_t* seen_j, int64_t* seen_pos) {
  static const uint8_t some_shares[1] = {0};
  std::vector<Secret> secrets(count);
  for (size_t i = 0; i < count; ++i) secrets[i] = Secret{pos_off[i] < 0 ? nullptr : pos + pos_off[i], has_shares[i] ? some_shares : nullptr, m[i]};
  bool fits = true;
  const many::SecretPlans p = many::plan_secrets(
      secrets.data(), count, cap_each, cap_run, host_threads, [&](size_t n) { fits = n <= slots_cap; },
      [&](const int64_t* positions, size_t len, size_t j, size_t c) {
        if (!fits) return false;
        __atomic_fetch_add(&visits[c], 1, __ATOMIC_RELAXED);
        seen_m[c] = len;
        seen_j[c] = j;
        seen_pos[c] = positions[j];
        return positions[j] != fail_pos;
      });
  if (!fits) return -1;
  for (size_t i = 0; i < count; ++i) {
    kind[i] = (int)p.secret[i].kind;
    coef[i] = p.secret[i].coef;
    list_of[i] = p.list_of[i];
  }
  for (size_t l = 0; l < p.list_first.size(); ++l) {
    list_first[l] = p.list_first[l];
    list_m[l] = p.list_m[l];
  }
  *coefs = p.coefs;
  return (long)p.list_first.size();
}

// the tile table of boxes of n[] shares; returns the words written, -1 when out[] (cap words) is too short
long many_tiles_c(const size_t* n, size_t boxes, size_t tile, size_t stride, uint32_t* out, size_t cap) {
  std::vector<uint32_t> t;
  many::tile_table(n, boxes, tile, stride, t);
  if (t.size() > cap) return -1;
  if (!t.empty()) memcpy(out, t.data(), t.size() * 4);
  return (long)t.size();
}
}

#ifdef MANY_HOST_MAIN
#include <stdio.h>

int main() {
  int bad = 0;
  // the walk: skip, aside and alone items between grouped ones, both caps met exactly and passed by one, a key change
  const int kinds[] = {3, 0, 3, 1, 3, 2, 3, 3, 3, 3, 3};
  const size_t a[] = {16, 0, 16, 0, 1, 99, 5, 5, 32, 31, 2}, b[] = {1, 0, 1, 0, 1, 1, 16, 17, 1, 1, 1};
  const int64_t keys[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 7};
  int64_t events[64];
  long words = 0;
  for (long fail_at = -1; fail_at < 8; ++fail_at) {
    const int rc = many_walk_c(11, kinds, a, b, keys, 32, 32, fail_at, 5, events, 64, &words);
    if (words < 0 || (fail_at < 0 && rc != 0)) ++bad;
  }
  // the plan: equal lists, a permuted one, a prefix, refused and single secrets; totals on both sides of parallel_for's threshold
  for (size_t len : {1, 7, 128, 300})
    for (int threads : {0, 1, 2, 16}) {
      std::vector<int64_t> pos(3 * len);
      for (size_t i = 0; i < len; ++i) {
        pos[i] = (int64_t)i + 1;
        pos[len + i] = (int64_t)(len - i);
        pos[2 * len + i] = i == 0 ? 0 : (int64_t)i;
      }
      const long off[] = {0, (long)len, 0, -1, (long)(2 * len), 0, 0};
      const size_t m[] = {len, len, len, len, len, len > 1 ? len - 1 : 1, (size_t)1 << 31};
      const int shares[] = {1, 1, 1, 1, 1, 1, 1};
      int kind[7], visits[1024] = {0};
      size_t coef[7], list_of[7], list_first[7], list_m[7], coefs = 0, seen_m[1024], seen_j[1024];
      int64_t seen_pos[1024];
      const long lists = many_plan_c(7, pos.data(), off, m, shares, 256, 1 << 18, threads, 3, kind, coef, list_of, list_first, list_m,
                                     &coefs, 1024, visits, seen_m, seen_j, seen_pos);
      if (lists < 0) ++bad;
      for (size_t c = 0; c < coefs; ++c) bad += visits[c] != 1;
    }
  // the tile table at both strides
  const size_t n[] = {1, 15, 16, 17, 33, 64, 65, 129};
  uint32_t out[256];
  if (many_tiles_c(n, 8, 16, 4, out, 256) != 4 * 26) ++bad;
  if (many_tiles_c(n, 8, 64, 3, out, 256) != 3 * 11) ++bad;
  if (many_threads_c(0, 0, 64) != 1 || many_threads_c(99, 0, 64) != 16) ++bad;
  printf(bad ? "many_host_shim: %d checks failed\n" : "many_host_shim: ok\n", bad);
  return bad ? 1 : 0;
}
#endif
