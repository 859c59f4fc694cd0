"""CPU side of the grouped path of mpvss_ec_verify_many: the model of the run rule and of the tile table
(tests/ec_many_boxes_cases.py) is held to its claims, and the header, the Python binding and the built library agree on the two
new entry points."""
import ctypes as C
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import ec_many_boxes_cases as MB
from ec_many_boxes_cases import Shape

NEW = ("mpvss_ctx_set_ec_box_groups", "mpvss_ec_verify_many_stats")


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_entry_points():
    from mpvss_rs_amd import capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "mpvss_hip.h")).read()
    lib = capi.load_library()
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in capi.EXPORTED_SYMBOLS, sym
        assert hasattr(lib, sym), sym
    assert hasattr(capi.Engine, "set_ec_box_groups") and hasattr(capi.Engine, "ec_verify_many_stats")


def test_no_context_is_refused_and_writes_nothing():
    from mpvss_rs_amd import capi
    lib = capi.load_library()
    p, g, s = C.c_ulonglong(11), C.c_ulonglong(12), C.c_ulonglong(13)
    assert lib.mpvss_ec_verify_many_stats(None, C.byref(p), C.byref(g), C.byref(s)) == -1
    assert (p.value, g.value, s.value) == (11, 12, 13)
    assert lib.mpvss_ec_verify_many_stats(None, None, None, None) == -1
    for mode in (0, 1, 2):
        assert lib.mpvss_ctx_set_ec_box_groups(None, mode) == -1


# ---- the tile table ----------------------------------------------------------------------------------------------------
def random_run(rng, boxes):
    return [Shape(rng.choice([1, 2, 5, 63, 64, 65, 100, 127, 128, 129, 1000, 4095]), rng.choice([1, 2, 3, 17, 34])) for _ in range(boxes)]


@pytest.mark.parametrize("run", [MB.TILE_SHAPES, MB.CHUNK_SHAPES[:2], [Shape(4095, 4095), Shape(1, 1)]] +
                         [random_run(random.Random(s), 1 + s % 9) for s in range(20)], ids=lambda r: f"{len(r)}boxes")
def test_tiles_cover_every_share_once_and_span_no_box(run):
    tl, bt = MB.tiles(run)
    first = [sum(b.n for b in run[:k]) for k in range(len(run) + 1)]
    seen = [0] * first[-1]
    for box, start, live in tl:
        assert 1 <= live <= MB.TILE
        assert first[box] <= start and start + live <= first[box + 1]          # inside ONE box
        assert (start - first[box]) % MB.TILE == 0
        for i in range(start, start + live):
            seen[i] += 1
    assert seen == [1] * first[-1]
    assert [b for b, _, _ in tl] == sorted(b for b, _, _ in tl)                # in box order: the concatenation's order
    assert len(tl) == sum((b.n + MB.TILE - 1) // MB.TILE for b in run)
    assert bt == [(sum(b.t for b in run[:k]), run[k].t) for k in range(len(run))]


def test_the_tile_shapes_are_the_edges_they_claim():
    assert sorted({b.n for b in MB.TILE_SHAPES}) == MB.TILE_N and sorted({b.t for b in MB.TILE_SHAPES}) == MB.TILE_T
    assert all(b.t <= b.n for b in MB.TILE_SHAPES)
    assert {live for _, _, live in MB.tiles(MB.TILE_SHAPES)[0]} == {1, 2, 63, 64}
    assert MB.runs(MB.TILE_SHAPES) == ([list(range(len(MB.TILE_SHAPES)))], [])
    assert [len(p) for p in MB.POSITION_LISTS] == [5, 6, 3, 5, 3] and all(t <= len(p) for t, p in zip(MB.POSITION_T, MB.POSITION_LISTS))
    flat = [x for p in MB.POSITION_LISTS for x in p]
    assert 0 in flat and 1 in flat and (1 << 40) in flat and min(flat) < 0 and any(1 << 20 < x < 1 << 30 for x in flat)


# ---- the run rule ------------------------------------------------------------------------------------------------------
def test_4095_is_small_and_4096_is_not():
    assert MB.small(Shape(4095, 4095)) and MB.small(Shape(1, 1))
    assert not MB.small(Shape(4096, 3)) and not MB.small(Shape(5, 4096))
    assert not MB.small(Shape(0, 3)) and not MB.small(Shape(5, 0)) and not MB.small(Shape(5, 3, False))
    assert MB.runs([Shape(4095, 3), Shape(4095, 3)]) == ([[0, 1]], [])
    assert MB.runs([Shape(4095, 3), Shape(4096, 3), Shape(5, 3)]) == ([], [0, 1, 2])
    assert MB.runs([Shape(5, 3), Shape(5, 3), Shape(4096, 16), Shape(5, 3), Shape(5, 3)]) == ([[0, 1], [3, 4]], [2])


def test_what_splits_a_run():
    s = Shape(5, 3)
    assert MB.runs([]) == ([], [])
    assert MB.runs([s]) == ([], [0])
    assert MB.runs([s, s, Shape(0, 3), s, s]) == ([[0, 1], [3, 4]], [2])                    # an empty box
    assert MB.runs([s, s, Shape(5, 3, False), s]) == ([[0, 1]], [2, 3])                     # a malformed one, then a run of one
    assert MB.stats([s, s, Shape(0, 3), s, s]) == {"passes": 2, "grouped_boxes": 4, "single_boxes": 0}
    assert MB.stats([s, s, Shape(5, 3, False), s]) == {"passes": 1, "grouped_boxes": 2, "single_boxes": 1}
    assert MB.stats([s, s, s], refused=(1,)) == {"passes": 1, "grouped_boxes": 2, "single_boxes": 0}
    assert MB.stats([s, s], refused=(0, 1)) == {"passes": 0, "grouped_boxes": 0, "single_boxes": 0}


@pytest.mark.parametrize("seed", range(30))
def test_runs_are_maximal_and_within_the_caps(seed):
    rng = random.Random(seed)
    cap = rng.choice([16, 32, 100, 1000])
    boxes = [Shape(rng.choice([0, 1, 3, 5, 15, 16, 17, 31, 32, 33, 99, 100]), rng.choice([0, 1, 2, 3, 16, 17, 33]), rng.random() > 0.1)
             for _ in range(40)]
    passes, singles = MB.runs(boxes, cap)
    assert sorted([i for p in passes for i in p] + singles) == list(range(len(boxes)))      # every box exactly once
    for p in passes:
        assert len(p) >= 2 and p == list(range(p[0], p[-1] + 1))
        assert all(MB.small(boxes[i], cap) for i in p)
        assert sum(boxes[i].n for i in p) <= cap and sum(boxes[i].t for i in p) <= cap
        # maximal: the box after the pass, if small, would overfill it; the box before it did not fit the run before
        nxt = p[-1] + 1
        if nxt < len(boxes) and MB.small(boxes[nxt], cap):
            assert sum(boxes[i].n for i in p) + boxes[nxt].n > cap or sum(boxes[i].t for i in p) + boxes[nxt].t > cap
    for i in singles:
        if MB.small(boxes[i], cap) and i + 1 < len(boxes) and MB.small(boxes[i + 1], cap) and i + 1 in singles:
            assert boxes[i].n + boxes[i + 1].n > cap or boxes[i].t + boxes[i + 1].t > cap   # two small neighbours stay apart only for a cap


@pytest.mark.parametrize("cap", [16, 32, 1000])
def test_the_caps_at_their_edges(cap):
    for fill, want in ((cap - 1, ([[0, 1]], [])), (cap, ([[0, 1]], [])), (cap + 1, ([], [0, 1]))):
        assert MB.runs([Shape(fill - 7, 1), Shape(7, 1)], cap) == want                      # shares
        assert MB.runs([Shape(cap // 2, fill - 7), Shape(cap // 2, 7)], cap) == want        # commitments
    # a third box that overfills starts the next run
    assert MB.runs([Shape(cap // 2, 1), Shape(cap // 2, 1), Shape(1, 1), Shape(1, 1)], cap) == ([[0, 1], [2, 3]], [])
    assert MB.runs([Shape(cap // 2, 1), Shape(cap // 2, 1), Shape(1, 1)], cap) == ([[0, 1]], [2])
    assert not MB.small(Shape(cap + 1, 1), cap) and MB.small(Shape(cap, cap), cap)


def test_the_chunk_shapes_fill_31_32_and_33():
    passes, singles = MB.runs(MB.CHUNK_SHAPES, MB.CHUNK)
    assert passes == MB.CHUNK_PASSES and singles == [2, 5, 6, 7, 8]
    assert [sum(MB.CHUNK_N[i] for i in p) for p in passes] == [31, 32, 10]
    assert MB.CHUNK_N[6] + MB.CHUNK_N[7] == 33
    assert MB.stats(MB.CHUNK_SHAPES, MB.CHUNK) == MB.CHUNK_STATS
    assert all(t <= n or n == 0 for n, t in zip(MB.CHUNK_N, MB.CHUNK_T))
