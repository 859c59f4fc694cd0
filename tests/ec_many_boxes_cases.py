"""The run rule and the tile table of mpvss_ec_verify_many as a pure-Python model, and the shapes that
tests/test_gpu_ec_many_boxes.py sends through the call.  tests/test_ec_many_boxes_cases.py holds the model to its claims.

A box is modelled by Shape(n, t, ok): ok = False stands for whatever the host judges before anything is launched -- a null pointer
or a challenge that is not below the group order.  A box is *small* when 1 <= n < 4096, 1 <= t < 4096, n and t <= max_chunk and ok.
A run is a maximal stretch of consecutive small boxes that hold at most max_chunk shares and at most max_chunk commitments
together, found greedily from the left; a run of two or more boxes is one grouped pass, every other box takes a block slot of its
own.  A tile is up to 64 consecutive shares of ONE box: one workgroup of k_*_commit_eval_tiles."""
from collections import namedtuple

Shape = namedtuple("Shape", "n t ok", defaults=(True,))

BOX_MAX = 4096          # EC_GROUP_BOX_MAX: the bound below which the forward differences never apply (n >= 4096)
TILE = 64               # one wave of the 64-lane curve kernels
MAX_CHUNK = 1 << 18     # the library's default


def small(box, max_chunk=MAX_CHUNK):
    return bool(box.ok) and 1 <= box.n < BOX_MAX and 1 <= box.t < BOX_MAX and box.n <= max_chunk and box.t <= max_chunk


def runs(boxes, max_chunk=MAX_CHUNK):
    """(passes, singles): passes = [[indices of a grouped pass]], singles = the indices that take a block slot of their own (empty
    and malformed boxes included), both in box order"""
    passes, singles = [], []
    i = 0
    while i < len(boxes):
        if not small(boxes[i], max_chunk):
            singles.append(i)
            i += 1
            continue
        j, shares, cms = i, 0, 0
        while j < len(boxes) and small(boxes[j], max_chunk) and shares + boxes[j].n <= max_chunk and cms + boxes[j].t <= max_chunk:
            shares += boxes[j].n
            cms += boxes[j].t
            j += 1
        if j - i >= 2:
            passes.append(list(range(i, j)))
        else:
            singles.append(i)
        i = j
    return passes, singles


def tiles(run):
    """(tiles, boxes) of a run of shapes: tiles = [(box, first share in the concatenation, live count)], boxes = [(first commitment
    in the decoded array, t)]"""
    tl, bt = [], []
    s = c = 0
    for k, b in enumerate(run):
        bt.append((c, b.t))
        for off in range(0, b.n, TILE):
            tl.append((k, s + off, min(b.n - off, TILE)))
        s += b.n
        c += b.t
    return tl, bt


def stats(boxes, max_chunk=MAX_CHUNK, refused=()):
    """what mpvss_ec_verify_many_stats adds for one call over `boxes`: empty boxes and boxes turned down (malformed ones, and
    the indices in `refused`) are in none of the counts; a pass counts when it verified a box"""
    passes, singles = runs(boxes, max_chunk)
    good = [[i for i in p if i not in refused] for p in passes]
    return {"passes": sum(1 for g in good if g), "grouped_boxes": sum(len(g) for g in good),
            "single_boxes": sum(1 for i in singles if boxes[i].ok and boxes[i].n > 0 and boxes[i].t > 0 and i not in refused)}


# ---- the shapes of the GPU module --------------------------------------------------------------------------------------
# every edge of a tile (one lane, a wave short of one, full, one lane into the next, two full, one over) with t = 1 (no Horner
# step), 2, 3 and 17; t <= n, as the dealer asks
TILE_N = [1, 2, 63, 64, 65, 128, 129]
TILE_T = [1, 2, 3, 17]
TILE_SHAPES = [Shape(1, 1), Shape(2, 2), Shape(63, 3), Shape(64, 17), Shape(65, 1), Shape(128, 2), Shape(129, 17), Shape(2, 1),
               Shape(63, 17), Shape(64, 3), Shape(129, 1), Shape(65, 2), Shape(128, 3)]
# 0, 1, scattered below 2^30, 2^40 and a negative one (Scalar::from(position as u64): it wraps)
POSITION_LISTS = [
    [0, 1, 2, 3, 4],
    [1, 0, 977, (1 << 30) - 1, 123456789, 5],
    [(1 << 40), (1 << 40) + 3, 7],
    [-3, 5, 1, -1, (1 << 30) - 5],
    [3, 2, 1],
]
POSITION_T = [3, 4, 2, 3, 1]
# under MPVSS_MAX_CHUNK = 32 (shares per box; an empty box splits runs): a pass of 31 shares, a pass of exactly 32, then 16 + 17 =
# 33 shares, which no pass holds -- 16 is a run of one, 17 as well since 33 > max_chunk is not small -- and a closing pass
CHUNK = 32
CHUNK_N = [16, 15, 0, 16, 16, 0, 16, 17, 33, 5, 5]
CHUNK_T = [3, 15, 1, 16, 2, 1, 1, 3, 2, 5, 1]
CHUNK_SHAPES = [Shape(n, t) for n, t in zip(CHUNK_N, CHUNK_T)]
CHUNK_PASSES = [[0, 1], [3, 4], [9, 10]]
CHUNK_STATS = {"passes": 3, "grouped_boxes": 6, "single_boxes": 3}
