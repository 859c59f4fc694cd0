"""The builders and the reference of tests/modp_rt_reconstruct_cases.py against the oracle, so that
tests/test_gpu_modp_rt_reconstruct_edges.py cannot pass against a wrong expectation.  No GPU: the shares that the GPU module takes
from the handle's fixed-base call come from Python's pow here."""
import functools
import math

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_reconstruct_cases as K


@functools.lru_cache(maxsize=None)
def builder(key):
    return K.RtBuilder(key)


def oracle_mask(b, case):
    """O.reconstruct over a synthetic box with U = 0: the mask as an integer, or None"""
    sbs, box = K.synthetic_box(b.G, case)
    return O.reconstruct(b.G, sbs, box)


def holds_to_oracle(b, case, memo):
    """the reference and the oracle agree on the case; returns the reference's encoding or None"""
    got, want = b.reference(case, memo), oracle_mask(b, case)
    if got is None:
        assert want is None, (b.name, case.id)
    else:
        assert want == int.from_bytes(b.mask(got), "big"), (b.name, case.id)
    return got


def test_the_groups_are_what_the_table_says():
    for key in K.KEYS:
        b = builder(key)
        rounds = 24 if b.q < 2 ** 300 else 2
        assert b.q % 4 == 3 and H.miller_rabin(b.q, rounds) and H.miller_rabin(b.sub, rounds), key     # a safe prime
        assert pow(4, b.sub, b.q) == 1 and 4 % b.q != 1                          # g = 4 has order q'
        if b.EB == 256:
            assert H.width_for_bits(b.q.bit_length()) == b.lpl, key
        else:
            assert b.q.bit_length() == 3072 and b.lpl == 27
    assert builder("b40").q % 8 == 7 and builder("b64").q % 8 == 3
    assert pow(2, builder("b64").sub, builder("b64").q) == builder("b64").q - 1   # 2 is a non-residue there
    assert [builder(k).lpl for k in K.WIDTHS] == [5, 9, 18, 27]
    assert K.Q_1_MOD_4 % 4 == 1 and H.miller_rabin(K.Q_1_MOD_4)


@pytest.mark.parametrize("key", K.KEYS)
def test_identity_claims_equal_the_reference(key):
    """family A up to m = 33 and the mask cases: 4^P(0) is what the reference reconstructs (family B1 has a test of its own)"""
    b, memo = builder(key), {}
    cases = [b.shape_case(m) for m in b.shape_sizes(33)]
    assert len(cases) == (15 if b.sub > 33 else {"q23": 9, "q47": 12}[key])
    if key in K.MASK_KEYS:
        cases += b.mask_cases()
    for c in cases:
        assert c.expect[0] == "identity"
        assert b.reference(c, memo) == b.expected(c), (key, c.id)


@pytest.mark.parametrize("key", K.KEYS)
def test_reference_equals_oracle_on_small_positions(key):
    """wherever the oracle's coefficient loop over 1..max(positions) can run: shapes up to m = 9, family D"""
    b, memo = builder(key), {}
    for m in b.shape_sizes(9):
        assert holds_to_oracle(b, b.shape_case(m), memo) is not None
    if key not in K.SIGN_KEYS:
        return
    kinds = set()
    # (a pow of Python at 2048 / 3072 bits costs 20 / 70 ms and the oracle does one per share: there the m = 17 list goes through
    # it for one case of each kind of special share, the m = 5 list whole)
    few = ("swapped", "minus-one-neg", "unreduced-swapped", "q-neg")
    for m in K.SIGN_M:
        for c in b.sign_cases(m):
            if m == 17 and b.q.bit_length() > 1024 and not c.id.endswith(few):
                continue
            got = holds_to_oracle(b, c, memo)
            kinds.add(c.expect[0])
            assert got == b.expected(c, memo), (key, c.id)                      # a value with the builder's claim, or a refusal
    assert kinds == {"ref", "refuse"}


@pytest.mark.parametrize("key", sorted(K.TINY))
def test_tiny_moduli_counts_by_the_reference_alone(key):
    """family C: how many sets the reference reconstructs, how many it refuses, and how many of the first have a raw denominator
    that is 0 mod q' -- the sets a separate reduction of numerator and denominator refuses wrongly"""
    b, memo = builder(key), {}
    cases = b.tiny_cases()
    value = refused = gcd_sets = 0
    for c in cases:
        got = holds_to_oracle(b, c, memo)
        assert sorted(c.positions) == [int(x) for x in c.id[2:].split("-")]
        if got is None:
            refused += 1
            assert K.raw_denominator_vanishes(c.positions, b.sub), c.id          # (nothing else makes the reference refuse here)
        else:
            value += 1
            gcd_sets += K.raw_denominator_vanishes(c.positions, b.sub)
    assert (len(cases), value, refused, gcd_sets) == K.TINY_COUNTS[key]
    if key == "q23":
        one = next(c for c in cases if sorted(c.positions) == [1, 11, 12])       # 132/110, 6/5, 1/1
        assert b.reference(one, memo) is not None and K.raw_denominator_vanishes(one.positions, b.sub)


@pytest.mark.parametrize("key", K.POSITION_KEYS)
def test_large_positions_are_reconstructed_at_every_modulus(key):
    b, memo = builder(key), {}
    for m in K.POSITION_M:
        cases = b.position_cases(m)
        xs = cases["asc"].positions
        assert max(xs) == 2 ** 63 - 1 and len({x % b.sub for x in xs}) == m      # different mod q' too
        if key == "b40":
            assert sum(x > b.q for x in xs) >= m - 5                             # all but the 32-bit edges are past q' and q
        if key == "b64":
            assert [x for x in xs if x > b.sub] == [2 ** 63 - 2, 2 ** 63 - 1]    # (q' is 0.965 * 2^63: the two ends are past it)
        for order, c in cases.items():
            assert sorted(c.positions) == xs and b.reference(c, memo) == b.expected(c), (key, m, order)


@pytest.mark.parametrize("key", K.SMALL_Q)
def test_positions_at_and_past_the_subgroup_order(key):
    """family B2: the reduced fraction decides"""
    b = builder(key)
    groups = b.small_q_cases()
    assert len(groups) == (4 if key == "b40" else 3)                             # (2 q' of the 64-bit prime is no int64)
    for cases in groups:
        for c in cases:
            assert all(1 <= x < 2 ** 63 for x in c.positions), c.id
            assert K.raw_denominator_vanishes(c.positions, b.sub), c.id
            got = b.reference(c)
            assert (got is None) == (c.expect[0] == "refuse"), (key, c.id)
        assert len({b.reference(c) for c in cases}) == 1
    gcd = groups[2]
    assert len(gcd) == 3 and len({tuple(c.positions) for c in gcd}) == 3 and sorted(gcd[0].positions) == [1, b.sub, 1 + b.sub]


def test_mask_reduction_is_exercised_on_both_sides():
    """at 40 and 64 bits a SHA-256 value is never below q; at 256 bits the seeded cases fall on both sides"""
    for key in K.SMALL_Q:
        b = builder(key)
        assert not any(b.hash_below_q(b.expected(c)) for c in b.mask_cases())
    b = builder("b256")
    sides = {b.hash_below_q(b.expected(c)) for c in b.mask_cases()}
    assert sides == {True, False}
    for c in b.mask_cases():
        gs = b.expected(c)
        h = int.from_bytes(O.sha256(O._be_min(int.from_bytes(gs, "big"))), "big")
        assert int.from_bytes(b.mask(gs), "big") == h % b.q


def test_sign_lists_and_their_lanes():
    b = builder("b64")
    for m in K.SIGN_M:
        xs = b.sign_positions(m)
        assert xs != sorted(xs) and xs != sorted(xs, reverse=True) and max(xs) <= 40
        lam = K.exact_lagrange(xs)
        assert K.lane_signs(xs) == [v < 0 for v in lam]
        pos_l, neg_l = b.sign_lanes(xs)
        assert len(pos_l) == 2 and len(neg_l) == 2
        assert all(lam[k] > 0 for k in pos_l) and all(lam[k] < 0 for k in neg_l)
    for key in K.SIGN_KEYS:
        b = builder(key)
        for m in K.SIGN_M:
            neg = K.lane_signs(b.sign_positions(m))
            for c in b.sign_cases(m):
                zero = [k for k, s in enumerate(c.shares) if int.from_bytes(s, "big") % b.q == 0]
                if c.expect[0] == "refuse":
                    assert len(zero) == 1 and neg[zero[0]], c.id
                else:
                    assert all(not neg[k] for k in zero), c.id
                    assert (c.expect[1] == bytes(b.EB)) == bool(zero), c.id
                assert all(len(s) == b.EB for s in c.shares)
            names = [c.id for c in b.sign_cases(m)]
            assert (f"D-m{m}-main-generator" in names) == (key == "b64")


def test_interleaved_order_changes_width_and_covers_every_pair():
    seq = K.interleaved_order()
    runs = seq[:4 * len(K.SHAPE_M)]
    assert {(k, m) for k, m in runs} == {(k, m) for k in K.WIDTHS for m in K.SHAPE_M}
    for (k0, m0), (k1, m1) in zip(seq, seq[1:]):
        assert k0 != k1 or m1 == 257                                              # (a new run starts at 257)
    for (k0, m0), (k1, m1) in zip(runs, runs[1:]):
        assert m0 > m1 or m1 == 257
    zig = seq[4 * len(K.SHAPE_M):]
    assert zig[:4] == [(K.WIDTHS[0], 257), (K.WIDTHS[3], 1), (K.WIDTHS[2], 256), (K.WIDTHS[1], 2)]


def test_refused_arguments_are_what_their_names_say():
    b = builder("b40")
    bad = b.refused_arguments()
    assert len(bad) == 8 and bad[-1] == ([], [])
    dup = bad[0][0]
    assert len(dup) == 257 and dup[0] == dup[-1] and len(set(dup)) == 256
    assert sorted(min(xs) for xs, _ in bad[1:7]) == [-1, -1, -1, 0, 0, 0]
    assert math.gcd((K.Q_1_MOD_4 - 1) // 2, 2) == 2
