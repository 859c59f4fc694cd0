"""tests/ec_dual_cases.py held to its claims on the CPU: the endomorphism classes of secp256k1 scalars (through the host
shim, which runs ec_glv.h itself), the recoded-nibble extremes (through the Python model of the recoding), the plain-C
reference against the Python oracle, and the lane discipline of the pools."""
import random

import pytest

import ec_dual_cases as D
import mpvss_oracle as O


@pytest.fixture(scope="module", params=D.NAMES)
def cs(request):
    return D.cases(request.param)


def test_secp256k1_classes_are_the_ten_and_the_class_grid_holds_every_pair():
    cs = D.cases("secp256k1")
    found = {cl for cl, _ in cs.classes}
    assert found == set(D.GLV_CLASSES), "the seeded search gives another class set: %r" % sorted(found)
    assert len(cs.classes) == 10
    for cl, k in cs.classes:
        assert 0 <= k < cs.order and D.glv_class(k) == cl
        m1, s1, m2, s2 = D.glv_split(k)
        assert ((-m1 if s1 else m1) + (-m2 if s2 else m2) * cs.lam - k) % cs.order == 0
    pairs = {(D.glv_class(row.r), D.glv_class(row.c)) for row in cs.class_grid}
    assert len(cs.class_grid) == 100 and pairs == {(a, b) for a in D.GLV_CLASSES for b in D.GLV_CLASSES}
    assert {a for a, _ in pairs} == {b for _, b in pairs} == set(D.GLV_CLASSES)
    # the class representatives are edge scalars as well: the digit grid meets them as r and as c
    edge = {k for _, k in cs.edge}
    assert all(k in edge for _, k in cs.classes)
    assert D.cases("ristretto255").classes == [] and D.cases("ristretto255").class_grid == []


def test_edge_scalars_are_reduced_and_hold_the_named_values(cs):
    vals = [k for _, k in cs.edge]
    assert all(0 <= k < cs.order for k in vals) and len(set(vals)) == len(vals)
    for k in (0, 1, 8, cs.order - 1, int("8" * 62, 16), int("f" * 63, 16) % cs.order):
        assert k in vals
    if cs.name == "secp256k1":
        lam = cs.lam
        assert lam == 0x5363ad4cc05c30e0a5261c028812645a122e22ea20816678df02967c1b23bd72
        for k in (lam, cs.order - lam, lam + 1, lam - 1, lam * lam % cs.order, (1 << 128) - 1, 1 << 128, 1 << 127):
            assert k in vals


def test_nibble_extremes_hold_under_the_recoding_model(cs):
    """digit -8 (nibble 0, table entry 8P) and digit +7 (nibble 15) at the first and last window of a recoded word,
    of the low half and at the top: on the full scalar (ristretto255's tables, both curves' comb) and, for secp256k1's
    tables, on the halves the shim returns."""
    full = {(w, nib) for _, scope, w, nib in cs.extremes if scope == "full"}
    for k, scope, w, nib in cs.extremes:
        assert 0 <= k < cs.order
        if scope == "full":
            assert D.recoded_nibbles(k)[w] == nib, (hex(k), w, nib)
        else:
            m1, _, m2, _ = D.glv_split(k)
            assert (D.recoded_nibbles(m1, 32)[w], D.recoded_nibbles(m2, 32)[w]) == nib, (hex(k), w, nib)
    if cs.name == "secp256k1":
        assert cs.unreachable == []
        assert full == {(w, nib) for w in D.EXTREME_WINDOWS for nib in (0, 15)} | {(64, 1)}
        halves = {(w, nib) for _, scope, w, nib in cs.extremes if scope == "halves"}
        assert halves == {(w, nib) for w in D.HALF_WINDOWS for nib in ((0, 15), (15, 0))}
    else:
        # a reduced ristretto255 scalar is below 2^253: recoded nibble 63 is 8 or 9 and the 65th digit 0 (the recoding is
        # monotone in k, so the two ends of the range decide it)
        assert [D.recoded_nibbles(k)[63:] for k in (0, cs.order - 1)] == [[8, 0], [9, 0]]
        assert sorted(cs.unreachable) == [(63, 0), (63, 15)]
        assert full == {(w, nib) for w in D.EXTREME_WINDOWS[:-1] for nib in (0, 15)}
    edge = {k for _, k in cs.edge}
    assert all(k in edge for k, _, _, _ in cs.extremes)


def test_digit_grid_meets_every_edge_scalar_as_r_and_as_c(cs):
    vals = {k for _, k in cs.edge}
    assert {row.r for row in cs.digit_grid} == vals == {row.c for row in cs.digit_grid}
    assert {(row.r, row.c) for row in cs.digit_grid} >= {(k, k) for k in vals}
    assert len(cs.digit_grid) == len(D.digit_pairs(len(vals))) <= max(D.DIGIT_GRID_MAX, len(vals))
    assert all(row.h1 == row.h2 != row.g2 for row in cs.digit_grid)
    assert len({row.h1 for row in cs.digit_grid}) == len(cs.digit_grid)              # P, Q differ per row
    for m in (1, 5, 28, 29, 55, 63, 200):
        pairs = D.digit_pairs(m)
        assert len(set(pairs)) == len(pairs)
        assert {i for i, _ in pairs} == {j for _, j in pairs} == set(range(m))


def test_base_grid_holds_every_triple_with_every_scalar_pair(cs):
    triples = cs.base_triples()
    assert len(triples) == (10 if cs.name == "secp256k1" else 9)
    assert len(cs.base_grid) == 7 * len(triples)
    n = cs.order
    assert {(r, c) for r, c in cs.base_scalars} == {(0, 0), (1, n - 1), (n - 1, n - 1), (0, cs.rand_c), (cs.rand_r, 0), (8, n - 8),
                                                    (cs.rand_r, cs.rand_c)}
    I, Gn = cs.ident, cs.gen
    shapes = set()
    for row in cs.base_grid:
        shapes.add((row.h1 == I, row.g2 == I, row.h2 == I, row.g2 == row.h1, row.h2 == row.h1, row.h1 == Gn, row.g2 == Gn))
    assert (True, True, True, True, True, False, False) in shapes          # I I I
    assert (False, False, False, True, True, False, False) in shapes       # P P P
    assert (False, False, False, True, False, True, True) in shapes        # G G -G
    e = cs.G.element_from_fixed
    for row in cs.base_grid:
        if "P P -P" in row.tag or "G G -G" in row.tag:
            assert cs.G.element_to_bytes(cs.G.element_inverse(e(row.g2))) == row.h2
        if "phi" in row.tag:
            x, y = e(row.g2)
            beta = 0x7ae96a2b657c07106e64479eac3434e99cf0497512f58995c1396c28719501ee
            assert e(row.h2) == (beta * x % O.SECP_P, y)


def test_reference_agrees_with_the_python_oracle(cs):
    """oracle/ec_ref.c against O.dleq_verifier_commitments: every row of the base grid, a seeded 5 % of the others, both
    choices of g1"""
    G = cs.G
    e = G.element_from_fixed
    rng = random.Random(0x5EED)
    rows = list(cs.base_grid)
    for grid in (cs.digit_grid, cs.class_grid, cs.pool, cs.pool_shared):
        rows += [row for row in grid if rng.random() < 0.05]
    for path, g1 in (("G", cs.gen), ("P", cs.p0)):
        for row in rows:
            a1, a2 = O.dleq_verifier_commitments(G, e(g1), e(row.h1), e(row.g2), e(row.h2), row.r, row.c)
            assert cs.expected(row, path) == (G.element_to_bytes(a1), G.element_to_bytes(a2)), (path, row.tag)
    for row in cs.pool[:3]:
        assert cs.mul(row.g1, row.r) == G.element_to_bytes(G.exp(e(row.g1), row.r))


def test_lane_pool_rows_of_neighbouring_lanes_differ_in_every_field(cs):
    assert len(cs.pool) == len(cs.pool_shared) == D.POOL
    fields = ("g1", "h1", "g2", "h2", "r", "c")
    for f in fields:
        assert len({getattr(row, f) for row in cs.pool}) == D.POOL
        if f != "c":
            assert len({getattr(row, f) for row in cs.pool_shared}) == D.POOL
    assert len({row.c for row in cs.pool_shared}) == 1                     # ONE challenge: it is the point of that pool
    for n in sorted(set(D.SHAPES) | set(D.EXTRACT_SHAPES)):
        for shared in (False, True):
            rows = cs.lane_rows(n, shared)
            assert len(rows) == n
            for i in range(n):
                for d in D.LANE_DISTANCES:
                    for j in (i - d, i + d):
                        if 0 <= j < n:
                            for f in fields[:5] if shared else fields:
                                assert getattr(rows[i], f) != getattr(rows[j], f), (n, i, j, f)
    # two shapes never start at the same pool row: a launch that reads the rows of another shape changes bytes
    assert len({cs.lane_rows(n)[0].tag for n in D.SHAPES}) == len(D.SHAPES)
