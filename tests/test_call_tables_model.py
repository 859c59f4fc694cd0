"""Integer model of the call-table program of a2 = y^r * Y^c (CallRows<R> / k_modp_rows2_dual_exp_pair, modp_pair_kernels.hip):
rows[j][d] = y^(d 2^(B j)), d < 64, j < R, B = 2048 / R; from weight 6 (NWIN - 1) down one squaring per bit, at weights divisible
by 6 a product per row with rows[j][window of r_j], the products of Y^c where the sliding-window schedule of c has a window.
The model must equal pow(y, r, q) * pow(Y, c, q) % q, count the operations the design's table states, and tell three mutants
(a row base off by one squaring, a digit off by one, the first row skipped) from the program."""
import random

import pytest

import mpvss_oracle as O

Q = O.ModpGroup().q


def sliding_schedule(c):
    """[(weight, odd digit)] from the top: windows of at most 4 bits that start and end in a set bit (odd powers 1, 3, .. 15 of Y)"""
    out, i = [], c.bit_length() - 1
    while i >= 0:
        if not (c >> i) & 1:
            i -= 1
            continue
        lo = max(i - 3, 0)
        while not (c >> lo) & 1:
            lo += 1
        out.append((lo, (c >> lo) & ((1 << (i - lo + 1)) - 1)))
        i = lo - 1
    return out


def build_rows(y, R, mutant=None):
    B = 2048 // R
    rows = []
    for j in range(R):
        e = B * j + (1 if mutant == "base" and j > 0 else 0)
        base = pow(y, 1 << e, Q)
        rows.append([pow(base, d, Q) for d in range(64)])
    return rows


def build_ops(R):
    """operations of the one-off build per key: (squarings, products); the conversion to Montgomery form is one product more"""
    return (R - 1) * (2048 // R), 62 * R


def row_program(y, r, Y, c, R, mutant=None):
    B = 2048 // R
    nwin = (B + 5) // 6
    top = 6 * (nwin - 1)
    rows = build_rows(y, R, mutant)
    sched = sliding_schedule(c)
    assert all(w <= top for w, _ in sched)

    def digit(j, w):
        width = min(6, B - 6 * w)
        d = (r >> (B * j + 6 * w)) & ((1 << width) - 1)
        return (d + 1) % 64 if mutant == "digit" else d

    ops = {"sq": 0, "row": 0, "c": 0, "close": 0}
    first = 1 if mutant == "skip0" else 0
    acc = rows[first][digit(first, nwin - 1)]          # the top window of the first row is loaded, not multiplied
    si = 0
    for cur in range(top, -1, -1):
        if cur != top:
            acc = acc * acc % Q
            ops["sq"] += 1
        if cur % 6 == 0:
            for j in range(first if cur != top else first + 1, R):
                acc = acc * rows[j][digit(j, cur // 6)] % Q
                ops["row"] += 1
        if si < len(sched) and sched[si][0] == cur:
            acc = acc * pow(Y, sched[si][1], Q) % Q
            ops["c"] += 1
            si += 1
    assert si == len(sched)
    ops["close"] = 1                                        # the product with plain 1 that leaves the Montgomery domain
    return acc, ops


def edge_exponents(R):
    B = 2048 // R
    ones = (1 << 2048) - 1
    return [0, 1, Q - 2, (1 << B) - 1, 1 << B, (1 << B) + 1, 1 << (2048 - B), ones, ones >> 2,
            ((1 << B) - 1) << (2048 - B),               # only the top row is set: every other row all zero
            (1 << B) - 1 + (1 << (2047)),
            sum(63 << (12 * k) for k in range(170))]      # all-ones windows alternating with all-zero windows


@pytest.mark.parametrize("R", [2, 4])
def test_row_program_equals_pow(R):
    rng = random.Random(100 + R)
    y, Y = pow(2, rng.randrange(Q - 1), Q), pow(4, rng.randrange(Q - 1), Q)
    cs = [rng.randrange(1 << 256), (1 << 256) - 1, 1, 0, 1 << 255]
    rs = edge_exponents(R) + [rng.randrange(1 << 2048) for _ in range(4)]
    for r in rs:
        for c in (cs if r in rs[:3] else cs[:2]):
            got, _ = row_program(y, r, Y, c, R)
            assert got == pow(y, r, Q) * pow(Y, c, Q) % Q, (R, hex(r)[:20], hex(c)[:20])
    for yy in (1, Q - 1):
        assert row_program(yy, rs[2], Y, cs[0], R)[0] == pow(yy, rs[2], Q) * pow(Y, cs[0], Q) % Q


@pytest.mark.parametrize("R,squarings,row_products", [(2, 1020, 341), (4, 510, 343)])
def test_operation_counts(R, squarings, row_products):
    """the design's table: R = 2 about 1 023 squarings and 394 products, R = 4 about 511 and 396 (with a 256-bit challenge's ~51
    sliding windows and the closing product); today 2 046 squarings, 394 products and 62 for y's window table"""
    rng = random.Random(7)
    c_products = []
    for _ in range(20):
        _, ops = row_program(3, rng.randrange(1 << 2048), 5, rng.randrange(1 << 255, 1 << 256), R)
        assert (ops["sq"], ops["row"], ops["close"]) == (squarings, row_products, 1)
        c_products.append(ops["c"])
    assert 45 <= sum(c_products) / len(c_products) <= 56
    total = row_products + sum(c_products) / len(c_products) + 1
    assert abs(total - (394 if R == 2 else 396)) <= 4
    assert squarings <= (1023 if R == 2 else 511)
    assert build_ops(R) == ((1024, 124) if R == 2 else (1536, 248))
    # issue slots per share at 85 per squaring and 122 per product: the model of the design (today: 2046 * 85 + 394 * 122 + 62 * 191)
    slots = squarings * 85 + total * 122
    assert slots < (136e3 if R == 2 else 93e3)


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("mutant", ["base", "digit", "skip0"])
def test_mutants_are_caught(R, mutant):
    rng = random.Random(5)
    y, Y = pow(2, rng.randrange(Q - 1), Q), pow(4, rng.randrange(Q - 1), Q)
    r, c = rng.randrange(1 << 2047, 1 << 2048), rng.randrange(1 << 256)
    want = pow(y, r, Q) * pow(Y, c, Q) % Q
    assert row_program(y, r, Y, c, R)[0] == want
    assert row_program(y, r, Y, c, R, mutant)[0] != want
