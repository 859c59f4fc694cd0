"""CPU unit tests of the plan of the fixed group's X path: mpvss_rs_amd/csrc/host_fd_plan.h is plain C++, so the very decisions
eval_x follows (path, chains, seed window, seeding levels, kernels, fault values), the inversion tree and the workspace sizes are
compiled here with g++ (tests/fd_plan_shim.cpp) and held to models that do not share its code: host_plan of
tests/test_fd_seed_window_model.py for the geometry, and below a transcription of the sizing loop eval_x had before the plan
existed, which the plan's sizes may never exceed."""
import ctypes as C
import itertools
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

from test_fd_seed_window_model import host_plan

LIB = os.path.join(HERE, "_build", "libfd_plan.so")
HORNER_ROW, HORNER, FD = range(3)                  # fdplan::Path
SEEDS_NONE, SEEDS_ROW, SEEDS_QUAD = range(3)       # fdplan::Seeds
STEP_QUAD, STEP_PAIR, STEP_PAIR_TILED = range(3)   # fdplan::Step
NUMBER = 72 * 4                                    # bytes of a number in Montgomery limbs
ROW_MAX_NUMBERS = 4096
PLAN = ("path fd device_positions S chain_len w0 seed0 m0 w1 two_level seeds1 seeds2 step1 step2 fault_table1 fault_step1 "
        "fault_table2 fault_step2 tile_steps").split()
BUFFERS = "xm xinv pre tot state gather hand_t hand_s".split()
BYTES = BUFFERS + "box_hand_t box_hand_s hand_t1_off hand_s1_off".split()

TS = (16, 17, 31, 32, 64, 255, 256, 257, 511, 512, 1024)


def counts(t):
    """the grid's share counts that the path admits at t commitments"""
    return sorted({c for c in (16 * t, 16 * t + 1, 4095, 4096, 8192, 16384, 65535, 65536, 131072) if c >= 16 * t})


def knobs(fd=1, min_shares=256, pair_min_t=512, pair_step=1, tile=0, tile_steps=64, l1=1, test_fault=0):
    """fdplan::Knobs as the shim takes them; the library's defaults but for min_shares, lowered as the GPU tests lower it"""
    return (C.c_int64 * 8)(fd, min_shares, pair_min_t, pair_step, tile, tile_steps, l1, test_fault)


def table_words(chains, t):
    return 7 * chains * t


def step_words(chains, t, length):
    return 3 * chains * (length + t)


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(HERE, "fd_plan_shim.cpp")
    csrc = os.path.join(HERE, "..", "mpvss_rs_amd", "csrc")
    deps = [src, os.path.join(csrc, "host_fd_plan.h"), os.path.join(csrc, "modp_limbs.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.fd_applies_c.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.fd_plan_c.restype = None
    lib.fd_plan_c.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.fd_tree_c.restype = C.c_long
    lib.fd_tree_c.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def plan(lib, k, t, cnt, boxes=1, busy=False, x_alone=False, direct=False, hpos=None):
    """(plan, its own Bytes, the sized Bytes) as dicts"""
    out, own, sized = (C.c_int64 * len(PLAN))(), (C.c_int64 * len(BYTES))(), (C.c_int64 * len(BYTES))()
    arr = (C.c_int64 * len(hpos))(*hpos) if hpos is not None else None
    lib.fd_plan_c(k, t, cnt, boxes, int(busy), int(x_alone), int(direct), arr, out, own, sized)
    return dict(zip(PLAN, out)), dict(zip(BYTES, own)), dict(zip(BYTES, sized))


def tree(lib, m):
    ms, pre_off, tot_off, totals = (C.c_int64 * 16)(), (C.c_int64 * 16)(), (C.c_int64 * 16)(), (C.c_int64 * 2)()
    nlev = lib.fd_tree_c(m, ms, pre_off, tot_off, 16, totals)
    assert nlev >= 0
    return list(ms[:nlev + 1]), list(pre_off[:nlev]), list(tot_off[1:nlev + 1]), totals[0], totals[1]


def tree_sizes(m):
    ms = [m]
    while ms[-1] > 1:
        ms.append((ms[-1] + 15) // 16)
    return ms


def former_sizing(t, cnt, boxes, busy, l1):
    """What eval_x allocated before the plan existed: its loop over three candidate chain counts -- the one taken, the pipelined one
    and the lone call's 16 -- each with a first seeding level whether or not any call would run one, and the later maximum with the
    configuration taken."""
    s_pipelined = max(max(min(2048 // t, cnt // 8192), cnt // 16384), 4)
    S = s_pipelined
    if 16 > S and (not busy or cnt >= 65536) and t <= 256:
        S = 16
    S = max(min(S, cnt // (4 * t)), 1)
    chain_len, m0 = (cnt + S - 1) // S, S * t
    two_level = S > 1 and (l1 >= 2 or (l1 == 1 and busy))
    s_cap = max(cnt // (4 * t), 1)
    need = dict.fromkeys(BUFFERS, 0)
    for sc in (S, min(s_pipelined, s_cap), min(16, s_cap) if t <= 256 else S):
        sc = max(sc, 1)
        m0c, clc = sc * t, (cnt + sc - 1) // sc
        ms = tree_sizes(m0c * boxes)
        l1t = table_words(1, t) * 4 if sc > 1 else 0
        l1s = step_words(1, t, m0c) * 4 if sc > 1 else 0
        cand = {"xinv": boxes * m0c * NUMBER, "pre": sum(ms[:-1]) * NUMBER, "tot": sum(ms[1:]) * NUMBER, "state": boxes * 2 * m0c * NUMBER,
                "hand_t": boxes * (table_words(sc, t) * 4 + l1t), "hand_s": boxes * (step_words(sc, t, clc) * 4 + l1s)}
        for f, v in cand.items():
            need[f] = max(need[f], v)
    hand_t = table_words(S, t) * 4 + (table_words(1, t) * 4 if two_level else 0)
    hand_s = step_words(S, t, chain_len) * 4 + (step_words(1, t, m0) * 4 if two_level else 0)
    need["hand_t"] = max(need["hand_t"], boxes * hand_t)
    need["hand_s"] = max(need["hand_s"], boxes * hand_s)
    need["xm"] = boxes * cnt * NUMBER
    need["gather"] = need["xinv"] if boxes > 1 else 0
    return need


@pytest.mark.parametrize("t", TS)
def test_geometry_tree_and_sizes_over_the_grid(shim, t):
    for cnt, boxes, busy, l1 in itertools.product(counts(t), (1, 2, 3), (False, True), (0, 1, 2)):
        k = knobs(l1=l1)
        where = (t, cnt, boxes, busy, l1)
        p, own, sized = plan(shim, k, t, cnt, boxes, busy)
        assert p["path"] == FD and p["fd"] == 1 and p["device_positions"] == 1, where
        assert (p["S"], p["chain_len"], p["w0"], p["seed0"], p["m0"], p["w1"]) == host_plan(t, cnt, busy), where
        assert p["seed0"] + p["m0"] <= cnt and p["S"] * p["chain_len"] >= cnt and p["w0"] >= 0, where
        assert p["two_level"] == int(p["S"] > 1 and (l1 == 2 or (l1 == 1 and busy))), where
        if p["two_level"]:
            assert p["S"] > 1 and 0 < p["w1"] and p["w1"] + t <= p["m0"], where
        # the tree of the larger inversion (every seed of every box) and of the first level's
        for m in (boxes * p["m0"], boxes * t):
            ms, pre_off, tot_off, pre, tot = tree(shim, m)
            assert ms == tree_sizes(m) and ms[0] == m and ms[-1] == 1, where
            assert pre_off == [sum(ms[:l]) for l in range(len(ms) - 1)] and pre == sum(ms[:-1]), where
            assert tot_off == [sum(ms[1:l]) for l in range(1, len(ms))] and tot == sum(ms[1:]), where
        # the plan's own bytes, from the stand-in word counts
        l1_t = table_words(1, t) * 4 if p["two_level"] else 0
        l1_s = step_words(1, t, p["m0"]) * 4 if p["two_level"] else 0
        ms = tree_sizes(boxes * p["m0"])
        assert own == {"xm": boxes * cnt * NUMBER, "xinv": boxes * p["m0"] * NUMBER, "pre": sum(ms[:-1]) * NUMBER,
                       "tot": sum(ms[1:]) * NUMBER, "state": boxes * 2 * p["m0"] * NUMBER,
                       "gather": boxes * p["m0"] * NUMBER if boxes > 1 else 0,
                       "hand_t1_off": table_words(p["S"], t) * 4, "hand_s1_off": step_words(p["S"], t, p["chain_len"]) * 4,
                       "box_hand_t": table_words(p["S"], t) * 4 + l1_t, "box_hand_s": step_words(p["S"], t, p["chain_len"]) * 4 + l1_s,
                       "hand_t": boxes * (table_words(p["S"], t) * 4 + l1_t),
                       "hand_s": boxes * (step_words(p["S"], t, p["chain_len"]) * 4 + l1_s)}, where
        # what the workspace is grown to: enough for this plan and for the one the slot meets when `busy` flips, never more than before
        other = plan(shim, k, t, cnt, boxes, not busy)
        former = former_sizing(t, cnt, boxes, busy, l1)
        for f in BUFFERS:
            assert max(own[f], other[1][f]) <= sized[f] <= former[f], (where, f)
        assert {f: sized[f] for f in BUFFERS} == {f: other[2][f] for f in BUFFERS}, where      # the same from either side of the flip
        assert all(sized[f] == own[f] for f in BYTES if f not in BUFFERS), where               # the layout is the plan's own


def test_the_two_plans_of_the_flip_test(shim):
    """t = 16, n = 1024 under the library's other defaults (tests/test_gpu_fd_plan_flip.py): a lone call has 16 chains and one
    seeding level, a box among others 4 chains and two levels with m0 = 64; the workspace of either is the larger of the two"""
    pos = list(range(1, 1025))
    lone, lone_b, lone_sized = plan(shim, knobs(), 16, 1024, hpos=pos)
    busy, busy_b, busy_sized = plan(shim, knobs(), 16, 1024, busy=True, hpos=pos)
    assert (lone["fd"], lone["S"], lone["m0"], lone["two_level"], lone["seeds2"]) == (1, 16, 256, 0, SEEDS_QUAD)
    assert (busy["fd"], busy["S"], busy["m0"], busy["two_level"], busy["seeds1"], busy["w1"]) == (1, 4, 64, 1, SEEDS_ROW, 24)
    for f in BUFFERS:
        assert lone_sized[f] == busy_sized[f] == max(lone_b[f], busy_b[f]), f
    assert lone_b["xinv"] == 4 * busy_b["xinv"] and lone_b["hand_s1_off"] != busy_b["hand_s1_off"]       # the plans do differ


def test_applies_at_every_threshold_edge(shim):
    k = knobs()                                      # min_shares 256
    run = lambda start, n: [start + i for i in range(n)]
    arr = lambda pos: (C.c_int64 * len(pos))(*pos)
    for t, cnt, want in ((15, 4096, 0), (16, 4096, 1), (1024, 16384, 1), (1025, 16400, 0), (16, 255, 0), (16, 256, 1), (64, 1023, 0),
                         (64, 1024, 1)):
        assert shim.fd_applies_c(k, t, cnt, None) == want, (t, cnt)
        assert shim.fd_applies_c(k, t, cnt, arr(run(1, cnt))) == want, (t, cnt)
    dflt = knobs(min_shares=4096)                    # the library's default
    assert shim.fd_applies_c(dflt, 16, 4095, None) == 0 and shim.fd_applies_c(dflt, 16, 4096, None) == 1
    assert shim.fd_applies_c(dflt, 256, 4095, None) == 0 and shim.fd_applies_c(dflt, 256, 4096, None) == 1
    assert shim.fd_applies_c(dflt, 257, 4096, None) == 0 and shim.fd_applies_c(dflt, 257, 16 * 257, None) == 1
    assert shim.fd_applies_c(knobs(fd=0), 16, 4096, None) == 0
    gap = run(1, 256)
    gap[255] += 1
    early = run(1, 256)
    early[1] = 3
    for pos, want in ((gap, 0), (early, 0), (run(0, 256), 1), (run(-1, 256), 0), (run((1 << 61) - 1, 256), 1), (run(1 << 61, 256), 0),
                      (list(reversed(run(1, 256))), 0)):
        assert shim.fd_applies_c(k, 16, 256, arr(pos)) == want, pos[:3]
        p, own, _ = plan(shim, k, 16, 256, hpos=pos)
        assert p["fd"] == want and p["path"] == (FD if want else HORNER_ROW) and p["device_positions"] == 0
        assert want or (p["S"] == 0 and not any(own.values()))


def test_paths_that_never_take_forward_differences(shim):
    k = knobs()
    for t, cnt, boxes, busy in itertools.product((16, 256), (4096, 4097, 65536), (1, 2), (False, True)):
        p, own, sized = plan(shim, k, t, cnt, boxes, busy, direct=True)
        assert p["fd"] == 0 and p["path"] == (HORNER_ROW if boxes == 1 and cnt <= ROW_MAX_NUMBERS else HORNER), (t, cnt, boxes)
        assert not any(own.values()) and not any(sized.values())
        assert plan(shim, k, t, cnt, boxes, busy)[0]["fd"] == 1
    # a shape the path does not admit: the row layout for a lone box of up to ROW_MAX_NUMBERS shares, Horner for a group of them
    for cnt, boxes, want in ((255, 1, HORNER_ROW), (255, 3, HORNER), (4096, 1, HORNER_ROW), (4097, 1, HORNER)):
        p = plan(shim, knobs(min_shares=1 << 20), 16, cnt, boxes)[0]
        assert (p["path"], p["fd"]) == (want, 0), (cnt, boxes)


def test_seed_kernels(shim):
    for l1, busy, x_alone in itertools.product((0, 1, 2), (False, True), (False, True)):
        p = plan(shim, knobs(l1=l1), 256, 65536, 1, busy, x_alone)[0]
        if p["two_level"]:
            assert (p["seeds1"], p["seeds2"]) == (SEEDS_ROW, SEEDS_NONE), (l1, busy, x_alone)
        else:
            assert (p["seeds1"], p["seeds2"]) == (SEEDS_NONE, SEEDS_ROW if x_alone and not busy else SEEDS_QUAD), (l1, busy, x_alone)


@pytest.mark.parametrize("tile", (0, 1, 2))
def test_fault_values_and_stepping_kernels(shim, tile):
    for fault, pair_step, t, busy in itertools.product(range(5), (0, 1), (256, 511, 512, 1024), (False, True)):
        pair_min_t = 512
        p = plan(shim, knobs(tile=tile, tile_steps=37, test_fault=fault, pair_step=pair_step, pair_min_t=pair_min_t, l1=2), t, 16 * t, 1,
                 busy)[0]
        where = (tile, fault, pair_step, t, busy)
        # level 2's launches get the variable raw, level 1's table 0, level 1's stepping 1 when the variable is 3
        assert (p["fault_table2"], p["fault_step2"], p["fault_table1"], p["fault_step1"]) == (fault, fault, 0, int(fault == 3)), where
        assert p["two_level"] == 1 and p["tile_steps"] == 37, where
        pair = bool(pair_step) and t >= pair_min_t
        tiled = pair and (tile == 2 or (tile == 1 and busy))
        for level, handed in (("step2", fault), ("step1", int(fault == 3))):
            want = STEP_PAIR_TILED if tiled and handed == 0 else STEP_PAIR if pair else STEP_QUAD
            assert p[level] == want, (where, level)
    # MPVSS_FD_PAIR_MIN_T moves the threshold
    assert plan(shim, knobs(pair_min_t=256), 256, 4096)[0]["step2"] == STEP_PAIR
    assert plan(shim, knobs(pair_min_t=257), 256, 4096)[0]["step2"] == STEP_QUAD
