"""Integer model of the call-table program of a2 = y^r * Y^c for any geometry (rows_dual_exp_pair<RowGeom<R, B, WIN>, true>,
modp_pair_kernels.hip): rows[j][d] = y^(d 2^(B j)), d < 2^WIN, j < R, B = 2048 / R; from weight TOP = WIN (NWIN - 1) down one
squaring per bit, at weights divisible by WIN a product per row with rows[j][window of r_j] (row 0's top window is loaded), and the
products of Y^c: where the sliding-window schedule of c has a window, or -- the per-share form -- the fixed nibbles of c at the
weights divisible by 4 below 256.

The geometry in use is (8, 5): NWIN = 52, TOP = 255, the top window of a row one bit wide, so that a window of c may lie anywhere
up to weight 255.  (8, 6) has TOP = 252 and loses the top window of c = 2^255: it must not be built (the program's static_assert).
The model must equal pow(y, r, q) * pow(Y, c, q) % q at the edges of the rows and of c, count 255 squarings, 415 row products and
one closing product, and tell four mutants from the program."""
import functools
import random

import pytest

from test_call_tables_model import Q, sliding_schedule

R8, W5 = 8, 5


def geometry(R, WIN):
    B = 2048 // R
    nwin = (B + WIN - 1) // WIN
    return B, nwin, WIN * (nwin - 1)


@functools.lru_cache(maxsize=8)
def build_rows(y, R, WIN, mutant=None):
    """the rows of one key: they depend on the key alone, as in the library, so the cases of one key share them"""
    B = 2048 // R
    rows = []
    for j in range(R):
        e = B * j + (1 if mutant == "base" and j > 0 else 0)
        base = pow(y, 1 << e, Q)
        rows.append([pow(base, d, Q) for d in range(1 << WIN)])
    return rows


def build_ops(R, WIN):
    """operations of the one-off build per key: (squarings, products); the conversion to Montgomery form is one product more"""
    return (R - 1) * (2048 // R), ((1 << WIN) - 2) * R


def row_program(y, r, Y, c, R, WIN, mutant=None, nibbles=False, check_top=True):
    B, nwin, top = geometry(R, WIN)
    rows = build_rows(y, R, WIN, mutant)
    sched = sliding_schedule(c)
    if check_top:
        assert all(w <= top for w, _ in sched)

    def digit(j, w):
        width = min(WIN, B - WIN * w)
        if mutant == "top_wide" and w == nwin - 1:
            width = WIN                                     # reads into the next row
        d = (r >> (B * j + WIN * w)) & ((1 << width) - 1)
        return (d + 1) % (1 << WIN) if mutant == "digit" else d

    ops = {"sq": 0, "row": 0, "c": 0, "close": 0}
    first = 1 if mutant == "skip0" else 0
    acc = rows[first][digit(first, nwin - 1)]          # the top window of the first row is loaded, not multiplied
    si = 0
    for cur in range(top, -1, -1):
        if cur != top:
            acc = acc * acc % Q
            ops["sq"] += 1
        if cur % WIN == 0:
            for j in range(first if cur != top else first + 1, R):
                acc = acc * rows[j][digit(j, cur // WIN)] % Q
                ops["row"] += 1
        if nibbles:
            if cur % 4 == 0 and cur < 256:
                acc = acc * pow(Y, (c >> cur) & 15, Q) % Q
                ops["c"] += 1
        elif si < len(sched) and sched[si][0] == cur:
            acc = acc * pow(Y, sched[si][1], Q) % Q
            ops["c"] += 1
            si += 1
    ops["close"] = 1                                        # the product with plain 1 that leaves the Montgomery domain
    return acc, ops


def edge_responses():
    ones = (1 << 2048) - 1
    out = [0, 1, Q - 2, ones]
    for k in range(1, 8):
        out += [(1 << (256 * k)) - 1, 1 << (256 * k), (1 << (256 * k)) + 1,
                1 << (256 * k + 255),                       # the 1-bit top window of row k
                ((1 << 256) - 1) << (256 * k)]              # only row k is set
    # all-ones windows alternating with all-zero windows, aligned to every row's own windows
    out.append(sum(31 << (256 * j + 10 * i) for j in range(8) for i in range(26)))
    return out


CHALLENGES = [(1 << 256) - 1, 1 << 255, (1 << 255) + 1, 9 << 252, 1, 0]


def want(y, r, Y, c):
    return pow(y, r, Q) * pow(Y, c, Q) % Q


def test_rows8_equal_pow_at_response_edges():
    rng = random.Random(85)
    y, Y = pow(2, rng.randrange(Q - 1), Q), pow(4, rng.randrange(Q - 1), Q)
    c = rng.randrange(1 << 255, 1 << 256)
    rs = edge_responses()
    assert len(rs) == 4 + 7 * 5 + 1
    for r in rs + [rng.randrange(1 << 2048) for _ in range(3)]:
        assert row_program(y, r, Y, c, R8, W5)[0] == want(y, r, Y, c), hex(r)[:24]
    for yy in (1, Q - 1):
        for r in (Q - 2, (1 << 2048) - 1, 1 << (256 * 3 + 255)):
            assert row_program(yy, r, Y, c, R8, W5)[0] == want(yy, r, Y, c)


@pytest.mark.parametrize("nibbles", [False, True], ids=["schedule", "nibbles"])
def test_rows8_equal_pow_at_challenge_edges(nibbles):
    rng = random.Random(86)
    y, Y = pow(2, rng.randrange(Q - 1), Q), pow(4, rng.randrange(Q - 1), Q)
    rs = [rng.randrange(1 << 2048), (1 << 2048) - 1, 1 << 255]
    for c in [rng.randrange(1 << 256)] + CHALLENGES:
        for r in rs:
            assert row_program(y, r, Y, c, R8, W5, nibbles=nibbles)[0] == want(y, r, Y, c), (hex(c)[:24], hex(r)[:24])


def test_operation_counts():
    """255 squarings, 415 row products, the closing product; with a 256-bit challenge's ~51 sliding windows under 80 K issue slots
    per share at 85 per squaring and 122 per product (two rows of 1 024 bits: 135 K).  The build: 1 792 squarings, 240 products."""
    rng = random.Random(7)
    c_products = []
    for _ in range(20):
        _, ops = row_program(3, rng.randrange(1 << 2048), 5, rng.randrange(1 << 255, 1 << 256), R8, W5)
        assert (ops["sq"], ops["row"], ops["close"]) == (255, 415, 1)
        c_products.append(ops["c"])
    mean_c = sum(c_products) / len(c_products)
    assert 45 <= mean_c <= 56
    assert 255 * 85 + (415 + mean_c + 1) * 122 < 80e3
    assert build_ops(R8, W5) == (1792, 240)
    _, ops = row_program(3, 5, 7, (1 << 256) - 1, R8, W5, nibbles=True)
    assert (ops["sq"], ops["row"], ops["c"]) == (255, 415, 64)


def test_schedule_weights_fit_five_bit_windows_only():
    """TOP = 255 for (8, 5): every window of a 256-bit c fits.  (8, 6): TOP = 252, and the one window of 2^255 lies above it -- the
    program would start below it and drop it."""
    assert geometry(8, 5) == (256, 52, 255)
    assert geometry(8, 6) == (256, 43, 252)
    rng = random.Random(9)
    for c in [rng.randrange(1 << 256) for _ in range(50)] + CHALLENGES:
        assert all(0 <= w <= 255 for w, _ in sliding_schedule(c))
    assert sliding_schedule(1 << 255) == [(255, 1)]
    assert sliding_schedule((1 << 255) + 1) == [(255, 1), (0, 1)]
    y, Y, r = 3, 5, rng.randrange(1 << 2048)
    with pytest.raises(AssertionError):
        row_program(y, r, Y, 1 << 255, 8, 6)
    for c in (1 << 255, (1 << 255) + 1):
        assert row_program(y, r, Y, c, 8, 6, check_top=False)[0] != want(y, r, Y, c)
        assert row_program(y, r, Y, c, 8, 5)[0] == want(y, r, Y, c)
    assert row_program(y, r, Y, 9 << 252, 8, 6)[0] == want(y, r, Y, 9 << 252)       # (a top window AT 252 is still within reach)


@pytest.mark.parametrize("mutant", ["base", "digit", "skip0", "top_wide"])
def test_mutants_are_caught(mutant):
    rng = random.Random(5)
    y, Y = pow(2, rng.randrange(Q - 1), Q), pow(4, rng.randrange(Q - 1), Q)
    r, c = (1 << 2048) - 1 - rng.randrange(1 << 2040), rng.randrange(1 << 256)
    if mutant == "top_wide":
        r |= 1 << 256                                       # the lowest bit of row 1: what row 0's top window must not read
    assert row_program(y, r, Y, c, R8, W5)[0] == want(y, r, Y, c)
    assert row_program(y, r, Y, c, R8, W5, mutant)[0] != want(y, r, Y, c)
