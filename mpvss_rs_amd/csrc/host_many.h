// What the "many in one call" entry points share on the host (mpvss_modp_group_verify_many, mpvss_modp_group_reconstruct_many,
// mpvss_ec_verify_many, mpvss_ec_reconstruct_many): the host threads of a call, the walk that decides which items travel together,
// the position-list plan of the reconstruct calls and the tile table of a dense pass.  Plain C++: no HIP, no context, so that
// tests/test_many_host.py runs the very code the entry points run (tests/many_host_shim.cpp), on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "host_scalar.h"

namespace many {

// host threads of a call: what the caller asked for, or one per `per_thread` items of work; 1 .. 16, never the machine's count
inline int many_threads(int requested, size_t work, size_t per_thread) {
  const size_t nth = requested > 0 ? (size_t)requested : work / per_thread;
  return (int)std::min<size_t>(std::max<size_t>(nth, 1), 16);
}

// what the walk does with an item:
//   SKIP     nothing; an open run stays open (a malformed box, a refused secret: settled before the walk)
//   ASIDE    alone(i) at once; an open run stays open (an empty box: no launch)
//   ALONE    the open run is flushed, then alone(i) (an item that fits no run)
//   GROUPED  joins the open run, or ends it and starts the next
enum Kind { SKIP, ASIDE, ALONE, GROUPED };

struct Cost {
  size_t a, b;
};

// THE grouping decision of every *_many call.  Items 0 .. count-1 are visited in order.  A run is a maximal stretch of GROUPED
// items, SKIP and ASIDE items between them notwithstanding, whose costs sum to at most cap_a and cap_b and which joins(first item
// of the run, item) lets travel together; found greedily from the left, cut only at item boundaries.  A run of two or more items
// is pass(run) (the items' indices, ascending); a run of one is alone(i), like every item that fits no run.  The end of the walk
// flushes.  A nonzero return of alone or pass ends the walk with that code, and nothing is called after it.
//   kind_of(i) -> Kind, cost(i) -> Cost, joins(first, i) -> bool, alone(i) -> int, pass(const std::vector<size_t>&) -> int
template <class KindOf, class CostOf, class Joins, class Alone, class Pass>
int walk(size_t count, size_t cap_a, size_t cap_b, KindOf kind_of, CostOf cost, Joins joins, Alone alone, Pass pass) {
  std::vector<size_t> run;
  Cost sum{0, 0};
  auto flush = [&]() -> int {
    const int rc = run.size() == 1 ? alone(run[0]) : run.size() > 1 ? pass(run) : 0;
    run.clear();
    sum = Cost{0, 0};
    return rc;
  };
  for (size_t i = 0; i < count; ++i) {
    const Kind kind = kind_of(i);
    if (kind == SKIP) continue;
    if (kind == ALONE)
      if (const int rc = flush()) return rc;
    if (kind != GROUPED) {
      if (const int rc = alone(i)) return rc;
      continue;
    }
    const Cost c = cost(i);
    if (!run.empty() && (sum.a + c.a > cap_a || sum.b + c.b > cap_b || !joins(run[0], i)))
      if (const int rc = flush()) return rc;
    run.push_back(i);
    sum.a += c.a;
    sum.b += c.b;
  }
  return flush();
}

// ---- the position-list plan of a reconstruct_many call ----------------------------------------------------------------------

enum SecretKind { SECRET_REFUSED, SECRET_GROUPED, SECRET_SINGLE };

// what the host knows of a secret before anything is launched: its kind, and where the coefficients of its position list start in
// the call's arrays (npos for a secret that computes its own)
struct SecretPlan {
  SecretKind kind = SECRET_REFUSED;
  size_t coef = (size_t)-1;
};

struct SecretPlans {
  std::vector<SecretPlan> secret;        // per secret
  std::vector<size_t> list_of;           // per secret: the index of its position list (npos unless it was judged GROUPED)
  std::vector<size_t> list_first;        // per distinct list: its first coefficient; lists lie back to back
  std::vector<size_t> list_m;            // per distinct list: its length
  std::vector<const int64_t*> list_pos;  // per distinct list: its positions (the caller's memory, of the first secret that has it)
  size_t coefs = 0;                      // coefficients in all
};

// The arguments of every secret (Secret: positions_host, shares, m), as the one-secret call judges them, and the distinct position
// lists -- the sequences equal element by element: a permuted list is another list, coefficients belong to indices -- of the
// secrets that may travel in a pass.  A secret of more than cap_each or cap_run shares is SINGLE: too long for a pass, it computes
// its own coefficients on the one-secret path.  Every GROUPED secret still awaits the verdict on its list: plan_settle.
template <class Secret>
SecretPlans plan_lists(const Secret* secrets, size_t count, size_t cap_each, size_t cap_run) {
  SecretPlans p;
  p.secret.resize(count);
  p.list_of.assign(count, (size_t)-1);
  std::map<std::vector<int64_t>, size_t> lists;          // position list -> its index
  for (size_t i = 0; i < count; ++i) {
    const Secret& s = secrets[i];
    if (!s.positions_host || !s.shares || s.m == 0 || s.m > 0x7fffffff) continue;
    bool ok = true;
    for (size_t k = 0; k < s.m && ok; ++k) ok = s.positions_host[k] >= 1;
    if (!ok) continue;
    if (s.m > cap_each || s.m > cap_run) {
      p.secret[i].kind = SECRET_SINGLE;
      continue;
    }
    p.secret[i].kind = SECRET_GROUPED;
    const auto it = lists.emplace(std::vector<int64_t>(s.positions_host, s.positions_host + s.m), p.list_pos.size());
    if (it.second) {
      p.list_pos.push_back(s.positions_host);
      p.list_m.push_back(s.m);
      p.list_first.push_back(p.coefs);
      p.coefs += s.m;
    }
    p.list_of[i] = it.first->second;
  }
  return p;
}

// the verdict on the lists: every GROUPED secret learns where its coefficients start, and is refused when its list has none
// (list_ok[l] == 0: duplicate positions, a denominator without inverse)
inline void plan_settle(SecretPlans& p, const std::vector<char>& list_ok) {
  for (size_t i = 0; i < p.secret.size(); ++i) {
    if (p.secret[i].kind != SECRET_GROUPED) continue;
    const size_t l = p.list_of[i];
    p.secret[i].coef = p.list_first[l];
    if (!list_ok[l]) p.secret[i].kind = SECRET_REFUSED;
  }
}

// The Lagrange coefficients ONCE per distinct position list of a plan_lists plan on the host, then plan_settle.
//   sized(coefs): called once, before any coefficient, so that the caller can size its arrays
//   coefficient(positions, m, j, c) -> bool: coefficient j of a list into the caller's slot c; false: the list has none (duplicate
//     positions, a denominator without inverse), and every secret of that list is refused.  Called on
//     many_threads(host_threads, coefs, 64) threads, every (list, j) exactly once.
template <class Sized, class Coefficient>
void plan_host_coefficients(SecretPlans& p, int host_threads, Sized sized, Coefficient coefficient) {
  sized(p.coefs);
  std::vector<char> coef_ok(p.coefs, 0);
  // a coefficient costs m small products and one inversion at the modulus' width: a thread per 64 of them when the library chooses
  hsc::parallel_for(p.coefs, many_threads(host_threads, p.coefs, 64), [&](size_t lo, size_t hi) {
    size_t l = std::upper_bound(p.list_first.begin(), p.list_first.end(), lo) - p.list_first.begin() - 1;
    for (size_t c = lo; c < hi; ++c) {
      while (l + 1 < p.list_first.size() && p.list_first[l + 1] <= c) ++l;
      coef_ok[c] = coefficient(p.list_pos[l], p.list_m[l], c - p.list_first[l], c) ? 1 : 0;
    }
  });
  std::vector<char> list_ok(p.list_m.size(), 0);
  for (size_t l = 0; l < list_ok.size(); ++l) {
    const auto first = coef_ok.begin() + p.list_first[l], last = first + p.list_m[l];
    list_ok[l] = std::find(first, last, 0) == last;
  }
  plan_settle(p, list_ok);
}

// plan_lists and plan_host_coefficients: the whole plan of a call whose coefficients are the host's
template <class Secret, class Sized, class Coefficient>
SecretPlans plan_secrets(const Secret* secrets, size_t count, size_t cap_each, size_t cap_run, int host_threads, Sized sized,
                         Coefficient coefficient) {
  SecretPlans p = plan_lists(secrets, count, cap_each, cap_run);
  plan_host_coefficients(p, host_threads, sized, coefficient);
  return p;
}

// the walk of a reconstruct_many call over its plan: refused secrets are settled and end no pass, costs are (m, 0)
template <class Secret, class Alone, class Pass>
int walk_secrets(const Secret* secrets, const std::vector<SecretPlan>& plan, size_t cap_run, Alone alone, Pass pass) {
  return walk(
      plan.size(), cap_run, 0,
      [&](size_t i) { return plan[i].kind == SECRET_REFUSED ? SKIP : plan[i].kind == SECRET_SINGLE ? ALONE : GROUPED; },
      [&](size_t i) { return Cost{secrets[i].m, 0}; }, [](size_t, size_t) { return true; }, alone, pass);
}

// ---- the tile table of a dense pass -------------------------------------------------------------------------------------------

// A tile is up to `tile` consecutive shares of ONE box: one workgroup of the *_commit_eval_tiles kernels.  Appends
// {box, first share in the concatenation, live count} and zeros up to `stride` words for every tile of the boxes' share counts
// n[0 .. boxes), in box order.
inline void tile_table(const size_t* n, size_t boxes, size_t tile, size_t stride, std::vector<uint32_t>& out) {
  size_t first = 0;
  for (size_t k = 0; k < boxes; ++k) {
    for (size_t off = 0; off < n[k]; off += tile) {
      const uint32_t row[3] = {(uint32_t)k, (uint32_t)(first + off), (uint32_t)std::min(n[k] - off, tile)};
      out.insert(out.end(), row, row + 3);
      out.insert(out.end(), stride - 3, 0u);
    }
    first += n[k];
  }
}

}  // namespace many
