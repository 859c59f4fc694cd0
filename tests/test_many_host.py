"""CPU unit tests of what the four *_many entry points share on the host: mpvss_rs_amd/csrc/host_many.h is plain C++, so the very
walk that decides which items travel together, the position-list plan of the reconstruct calls, the tile table of a dense pass and
the thread count of a call are compiled here with g++ (tests/many_host_shim.cpp) and compared with pure-Python models: walk_model
below for the general walk, tests/ec_many_boxes_cases.py for the curve rule and the tiles."""
import ctypes as C
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import ec_many_boxes_cases as MB
import ec_reconstruct_many_cases as EC_REC
import modp_rt_reconstruct_many_cases as RT_REC
from ec_many_boxes_cases import Shape

LIB = os.path.join(HERE, "_build", "libmany_host.so")
SKIP, ASIDE, ALONE, GROUPED = range(4)            # many::Kind
REFUSED, SEC_GROUPED, SINGLE = range(3)           # many::SecretKind
NPOS = (1 << 64) - 1


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(HERE, "many_host_shim.cpp")
    csrc = os.path.join(HERE, "..", "mpvss_rs_amd", "csrc")
    deps = [src, os.path.join(csrc, "host_many.h"), os.path.join(csrc, "host_scalar.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.many_threads_c.argtypes = [C.c_int, C.c_size_t, C.c_size_t]
    lib.many_walk_c.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_long, C.c_int,
                                C.c_void_p, C.c_size_t, C.c_void_p]
    lib.many_plan_c.restype = C.c_long
    lib.many_plan_c.argtypes = [C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t, C.c_size_t, C.c_int, C.c_int64] + [C.c_void_p] * 6 + \
                               [C.c_size_t] + [C.c_void_p] * 4
    lib.many_tiles_c.restype = C.c_long
    lib.many_tiles_c.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]
    return lib


# ---- the walk ------------------------------------------------------------------------------------------------------------
def walk_model(kinds, a, b, keys, cap_a, cap_b, fail_at=-1, fail_code=0):
    """(code, events) of many::walk: events = ("alone", i) and ("pass", [indices]) in the order the callbacks are called; the
    fail_at-th call returns fail_code, which ends the walk"""
    events, run, sa, sb = [], [], 0, 0

    def call(ev):
        events.append(ev)
        return fail_code if len(events) - 1 == fail_at else 0

    def flush():
        nonlocal run, sa, sb
        rc = call(("alone", run[0])) if len(run) == 1 else call(("pass", list(run))) if run else 0
        run, sa, sb = [], 0, 0
        return rc

    for i, kind in enumerate(kinds):
        if kind == SKIP:
            continue
        if kind == ALONE:
            rc = flush()
            if rc:
                return rc, events
        if kind != GROUPED:
            rc = call(("alone", i))
            if rc:
                return rc, events
            continue
        if run and (sa + a[i] > cap_a or sb + b[i] > cap_b or keys[run[0]] != keys[i]):
            rc = flush()
            if rc:
                return rc, events
        run.append(i)
        sa += a[i]
        sb += b[i]
    return flush(), events


def walk(shim, kinds, a, b, keys, cap_a, cap_b, fail_at=-1, fail_code=0):
    n = len(kinds)
    cap = 3 * n + 4
    ev = (C.c_int64 * cap)()
    words = C.c_long(0)
    rc = shim.many_walk_c(n, (C.c_int * max(n, 1))(*kinds), (C.c_size_t * max(n, 1))(*a), (C.c_size_t * max(n, 1))(*b),
                          (C.c_int64 * max(n, 1))(*keys), cap_a, cap_b, fail_at, fail_code, ev, cap, C.byref(words))
    assert words.value >= 0
    events, at = [], 0
    while at < words.value:
        if ev[at] == 0:
            events.append(("alone", ev[at + 1]))
            at += 2
        else:
            events.append(("pass", list(ev[at + 1:at + 1 + ev[at]])))
            at += 1 + ev[at]
    return rc, events


def both(shim, kinds, a, b, keys, cap_a, cap_b, **kw):
    got = walk(shim, kinds, a, b, keys, cap_a, cap_b, **kw)
    assert got == walk_model(kinds, a, b, keys, cap_a, cap_b, **kw)
    return got


def ec_walk(shim, boxes, cap):
    """the walk as mpvss_ec_verify_many calls it: a box that is not small is ALONE, the costs are (n, t) against cap and cap"""
    kinds = [GROUPED if MB.small(b, cap) else ALONE for b in boxes]
    rc, events = both(shim, kinds, [b.n for b in boxes], [b.t for b in boxes], [0] * len(boxes), cap, cap)
    assert rc == 0
    return [e[1] for e in events if e[0] == "pass"], [e[1] for e in events if e[0] == "alone"], events


def test_walk_curve_rule_on_the_chunk_shapes(shim):
    passes, alone, _ = ec_walk(shim, MB.CHUNK_SHAPES, MB.CHUNK)
    assert passes == MB.CHUNK_PASSES
    assert all(len(p) >= 2 for p in passes)
    # single_boxes counts the boxes outside the passes that the pipeline verified: those with shares
    assert sum(1 for i in alone if MB.CHUNK_SHAPES[i].n > 0) == MB.CHUNK_STATS["single_boxes"]
    assert {"passes": len(passes), "grouped_boxes": sum(map(len, passes))} == {k: MB.CHUNK_STATS[k] for k in ("passes", "grouped_boxes")}


def test_walk_curve_rule_equals_the_look_ahead_model(shim):
    rng = random.Random(20261020)
    sizes = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096]
    for case in range(200):
        boxes = [Shape(rng.choice(sizes), rng.choice(sizes), rng.random() < 0.85) for _ in range(rng.randrange(0, 24))]
        for cap in (32, 1 << 18):
            passes, alone, events = ec_walk(shim, boxes, cap)
            assert (passes, sorted(alone)) == MB.runs(boxes, cap), (case, cap)
            # the boxes are settled in order: every event lies behind the one before it, a pass is a contiguous range
            firsts = [e[1] if e[0] == "alone" else e[1][0] for e in events]
            assert firsts == sorted(firsts)
            assert all(p == list(range(p[0], p[-1] + 1)) for p in passes)


@pytest.mark.parametrize("cases", [RT_REC, EC_REC], ids=["modp_rt", "ec"])
def test_walk_reconstruct_rule_on_chunk_m(shim, cases):
    """refused -> skip, single (m > cap) -> alone, grouped -> grouped; costs (m, 0) against (cap, 0)"""
    assert cases.CHUNK_M == [16, 16, 3, 5, 33, 20, 7, 17] and cases.CHUNK == 32
    kinds = [ALONE if m > cases.CHUNK else GROUPED for m in cases.CHUNK_M]
    rc, events = both(shim, kinds, cases.CHUNK_M, [0] * 8, [0] * 8, cases.CHUNK, 0)
    assert rc == 0
    assert events == [("pass", [0, 1]), ("pass", [2, 3]), ("alone", 4), ("pass", [5, 6]), ("alone", 7)]
    passes = [e[1] for e in events if e[0] == "pass"]
    assert cases.CHUNK_STATS == {"passes": len(passes), "grouped_secrets": sum(map(len, passes)), "single_secrets": 2}


def test_walk_run_time_modp_rule(shim):
    cap = 32
    # a skip inside a run does not cut it; an aside item is settled at its position while the run stays open
    assert both(shim, [GROUPED, SKIP, GROUPED, ASIDE, GROUPED], [4, 0, 4, 0, 4], [1] * 5, [0] * 5, cap, cap) == \
        (0, [("alone", 3), ("pass", [0, 2, 4])])
    # an alone item cuts: the open run first, then the item
    assert both(shim, [GROUPED, GROUPED, ALONE, GROUPED], [4, 4, 99, 4], [1] * 4, [0] * 4, cap, cap) == \
        (0, [("pass", [0, 1]), ("alone", 2), ("alone", 3)])
    # a change of key set cuts, the same key set again does not join the run before
    assert both(shim, [GROUPED] * 5, [1] * 5, [1] * 5, [0, 0, 7, 7, 0], cap, cap) == (0, [("pass", [0, 1]), ("pass", [2, 3]), ("alone", 4)])
    # a sum equal to the cap joins, cap + 1 cuts: either cost on its own
    for which in (0, 1):
        for last, want in ((16, [("pass", [0, 1, 2])]), (17, [("pass", [0, 1]), ("alone", 2)])):
            cost = [8, 8, last]
            a, b = (cost, [1] * 3) if which == 0 else ([1] * 3, cost)
            assert both(shim, [GROUPED] * 3, a, b, [0] * 3, cap, cap) == (0, want), (which, last)
    # a run of one is alone, never a pass; nothing at all for no items, or only skipped ones
    assert both(shim, [GROUPED], [5], [5], [0], cap, cap) == (0, [("alone", 0)])
    assert both(shim, [SKIP, GROUPED, SKIP], [0, 5, 0], [0, 5, 0], [0] * 3, cap, cap) == (0, [("alone", 1)])
    assert both(shim, [], [], [], [], cap, cap) == (0, [])
    assert both(shim, [SKIP, SKIP], [0, 0], [0, 0], [0, 0], cap, cap) == (0, [])


def test_walk_ends_at_the_first_nonzero_code(shim):
    kinds = [GROUPED, GROUPED, ASIDE, ALONE, GROUPED, ALONE, GROUPED, GROUPED, GROUPED]
    a = [4, 4, 0, 99, 4, 99, 20, 20, 1]
    args = (kinds, a, [1] * 9, [0] * 9, 32, 32)
    rc, full = both(shim, *args)
    assert rc == 0
    # alone at once (aside), a pass flushed by an alone item, that item, a run of one flushed by one, a pass flushed by the cap, the end
    assert full == [("alone", 2), ("pass", [0, 1]), ("alone", 3), ("alone", 4), ("alone", 5), ("alone", 6), ("pass", [7, 8])]
    for fail_at in range(len(full)):
        rc, events = both(shim, *args, fail_at=fail_at, fail_code=-7 - fail_at)
        assert rc == -7 - fail_at
        assert events == full[:fail_at + 1]                      # nothing is called after the call that failed


# ---- the plan ------------------------------------------------------------------------------------------------------------
def plan(shim, secrets, cap_each=16384, cap_run=1 << 18, threads=0, fail_pos=-1):
    """secrets: (positions or None, has_shares[, m]) -> dict of the plan's arrays and of what the coefficient function saw"""
    count = len(secrets)
    flat, off, ms = [], [], []
    for s in secrets:
        pos = s[0]
        off.append(-1 if pos is None else len(flat))
        flat += pos or []
        ms.append(s[2] if len(s) > 2 else len(pos or []))
    slots = sum(m for m in ms if m <= len(flat)) + 1
    n1 = max(count, 1)
    kind, coef, list_of, list_first, list_m = (C.c_int * n1)(), (C.c_size_t * n1)(), (C.c_size_t * n1)(), (C.c_size_t * n1)(), (C.c_size_t * n1)()
    coefs = C.c_size_t(0)
    visits, seen_m, seen_j, seen_pos = (C.c_int * slots)(), (C.c_size_t * slots)(), (C.c_size_t * slots)(), (C.c_int64 * slots)()
    lists = shim.many_plan_c(count, (C.c_int64 * max(len(flat), 1))(*flat), (C.c_long * n1)(*off), (C.c_size_t * n1)(*ms),
                             (C.c_int * n1)(*[int(bool(s[1])) for s in secrets]), cap_each, cap_run, threads, fail_pos, kind, coef, list_of,
                             list_first, list_m, C.byref(coefs), slots, visits, seen_m, seen_j, seen_pos)
    assert lists >= 0
    n = coefs.value
    return {"kind": list(kind)[:count], "coef": list(coef)[:count], "list_of": list(list_of)[:count], "list_first": list(list_first)[:lists],
            "list_m": list(list_m)[:lists], "coefs": n, "visits": list(visits)[:n], "seen": list(zip(seen_m[:n], seen_j[:n], seen_pos[:n]))}


def test_plan_lists_are_equal_element_by_element(shim):
    base = [3, 1, 4, 15, 9]
    secrets = [(base, True), ([1, 3, 4, 9, 15], True), (base[:4], True), (list(base), True), (base[:4], True), ([2], True)]
    p = plan(shim, secrets)
    assert p["kind"] == [SEC_GROUPED] * 6
    assert p["list_of"] == [0, 1, 2, 0, 2, 3]                    # equal lists share one index; a permutation and a prefix are others
    assert p["list_m"] == [5, 5, 4, 1] and p["list_first"] == [0, 5, 10, 14] and p["coefs"] == 15      # back to back
    assert p["coef"] == [p["list_first"][l] for l in p["list_of"]]
    assert p["visits"] == [1] * 15


@pytest.mark.parametrize("threads", [1, 2, 16])
@pytest.mark.parametrize("total", [0, 1, 255, 256, 257, 1000])
def test_plan_visits_every_coefficient_once(shim, threads, total):
    """256 is hsc::parallel_for's threshold: below it one thread takes every coefficient"""
    rng = random.Random(total * 100 + threads)
    lengths, left = [], total
    while left:
        lengths.append(min(left, rng.choice([1, 2, 7, 64, 100])))
        left -= lengths[-1]
    lists = [[1 + 10000 * k + j for j in range(m)] for k, m in enumerate(lengths)]
    secrets = [(l, True) for l in lists] + [(l, True) for l in lists[::3]] + [(None, True), ([0, 1], True)]
    rng.shuffle(secrets)
    p = plan(shim, secrets, threads=threads)
    assert p["coefs"] == total and p["visits"] == [1] * total
    assert sorted(p["list_m"]) == sorted(lengths)
    assert p["list_first"] == [sum(p["list_m"][:l]) for l in range(len(lengths))]
    for i, s in enumerate(secrets):
        if p["kind"][i] != SEC_GROUPED:
            assert s[0] is None or 0 in s[0]
            continue
        first = p["list_first"][p["list_of"][i]]
        assert p["coef"][i] == first
        # slot first + j was asked for coefficient j of this very list
        assert p["seen"][first:first + len(s[0])] == [(len(s[0]), j, s[0][j]) for j in range(len(s[0]))]


def test_plan_failed_coefficient_refuses_its_list_alone(shim):
    secrets = [([1, 2, 3], True), ([4, 5, 6], True), ([1, 2, 3], True), ([5], True), ([4, 5, 6], True), ([4, 5], True)]
    p = plan(shim, secrets, fail_pos=6)
    assert p["kind"] == [SEC_GROUPED, REFUSED, SEC_GROUPED, SEC_GROUPED, REFUSED, SEC_GROUPED]
    assert p["coef"] == [0, 3, 0, 6, 3, 7]                       # a refused secret keeps the slot of its list
    assert p["visits"] == [1] * p["coefs"]
    assert plan(shim, secrets)["kind"] == [SEC_GROUPED] * 6


def test_plan_refused_and_single_secrets(shim):
    cap = 32
    ok = list(range(1, 6))
    secrets = [(ok, True), ([1, 0, 3], True), ([1, 2, -5], True), (None, True), (ok, False), ([], True), (ok, True, 0x80000000),
               (list(range(1, cap + 2)), True), (list(range(1, cap + 1)), True), (ok, True, 0x7fffffff + 1), (ok, True)]
    p = plan(shim, secrets, cap_each=16384, cap_run=cap)
    assert p["kind"] == [SEC_GROUPED, REFUSED, REFUSED, REFUSED, REFUSED, REFUSED, REFUSED, SINGLE, SEC_GROUPED, REFUSED, SEC_GROUPED]
    # only a grouped secret has a list and a slot: a single one computes its own coefficients
    for i, k in enumerate(p["kind"]):
        assert (p["coef"][i] == NPOS) == (k != SEC_GROUPED) and (p["list_of"][i] == NPOS) == (k != SEC_GROUPED)
    assert p["list_m"] == [5, cap] and p["coefs"] == 5 + cap
    # the cap of one secret on its own, below the cap of a run
    p = plan(shim, [(list(range(1, 9)), True), (list(range(1, 10)), True)], cap_each=8, cap_run=cap)
    assert p["kind"] == [SEC_GROUPED, SINGLE]


# ---- threads and tiles -----------------------------------------------------------------------------------------------------
def test_many_threads(shim):
    t = shim.many_threads_c
    assert t(0, 0, 64) == 1 and t(0, 63, 64) == 1 and t(0, 64, 64) == 1 and t(0, 128, 64) == 2
    for per in (64, 256, 512):
        assert t(0, 16 * per - 1, per) == 15 and t(0, 16 * per, per) == 16 and t(0, 1000 * per, per) == 16
    assert [t(r, w, 64) for r in (1, 16, 99) for w in (0, 1 << 20)] == [1, 1, 16, 16, 16, 16]
    assert t(-3, 640, 64) == 10                                  # anything below 1 leaves the choice to the library


def tile_rows(shim, counts, tile, stride):
    cap = stride * (sum(-(-n // tile) for n in counts) + 1)
    out = (C.c_uint32 * cap)(*([0xFFFFFFFF] * cap))
    words = shim.many_tiles_c((C.c_size_t * max(len(counts), 1))(*counts), len(counts), tile, stride, out, cap)
    assert words >= 0 and words % stride == 0 and list(out[words:]) == [0xFFFFFFFF] * (cap - words)
    return [tuple(out[r:r + stride]) for r in range(0, words, stride)]


def test_tile_table_of_the_curve_groups(shim):
    want, _ = MB.tiles(MB.TILE_SHAPES)
    assert tile_rows(shim, [s.n for s in MB.TILE_SHAPES], MB.TILE, 3) == want
    assert shim.many_tiles_c(None, 0, 64, 3, None, 0) == 0


def test_tile_table_of_the_run_time_groups(shim):
    counts = [1, 15, 16, 17, 33]
    rows = tile_rows(shim, counts, 16, 4)
    want, first = [], 0
    for k, n in enumerate(counts):
        want += [(k, first + off, min(n - off, 16), 0) for off in range(0, n, 16)]
        first += n
    assert rows == want and len(rows) == 1 + 1 + 1 + 2 + 3
    assert sum(r[2] for r in rows) == sum(counts)
