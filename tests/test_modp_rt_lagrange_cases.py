"""tests/modp_rt_lagrange_cases.py held to the references the other reconstruct tests rest on: reconstruct_cases.exact_lagrange
(exact fractions) for every exponent of every case, and ref_reconstruct over the oracle's group for what the exponents are for --
prod_i S_i^e_i is the reconstructed element.  No library, no GPU."""
import math
import random
from fractions import Fraction

import pytest

import modp_rt_lagrange_cases as LC
import modp_rt_reconstruct_cases as K
from reconstruct_cases import REFUSED, exact_lagrange, product, ref_reconstruct

_EXACT = {}


def exact(xs):
    key = tuple(xs)
    if key not in _EXACT:
        _EXACT[key] = exact_lagrange(xs)
    return _EXACT[key]


def from_fractions(q, xs):
    """the exponents from exact fractions, or None: what the reference computes at every modulus"""
    sub = (q - 1) // 2
    out = []
    for lam in exact(xs):
        try:
            mag = abs(lam.numerator) * pow(lam.denominator, -1, sub) % sub
        except ValueError:
            return None
        out.append(mag if (lam > 0 or mag == 0) else (q - 1) - mag)
    return out


def test_sizes_are_the_kernels_edges():
    assert (LC.TILE, LC.STAGE) == (16, 256)
    assert LC.SIZES == [1, 2, 3, 15, 16, 17, 255, 256, 257, 513] and LC.STEP_EDGE_SIZES == [258, 514]
    assert LC.WIDE_SIZES == [1, 2, 3, 17, 65] and LC.BIG_M == 4097
    assert [LC.HANDLES[k][1:] for k in LC.KEYS] == [(256, 5), (256, 9), (256, 18), (384, 27), (512, 36)]
    for key in LC.KEYS:
        ids = [cid for cid, _ in LC.cases(key)]
        assert len(set(ids)) == len(ids)
        for m in LC.sizes(key):
            assert f"shuffled-{m}" in ids and (m == 1 or (f"asc-{m}" in ids and f"desc-{m}" in ids))
        special = [xs for cid, xs in LC.cases(key) if cid.startswith("special-")]
        assert len(special) == 3 * len(LC.SPECIAL_M[key])
        assert all(2 ** 63 - 1 in xs and 1 in xs and 2 ** 32 in xs for xs in special)
        assert all(1 <= x < 2 ** 63 for _, xs in LC.cases(key) for x in xs)


@pytest.mark.parametrize("key", LC.KEYS)
def test_every_case_against_exact_fractions(key):
    q = LC.modulus(key)
    for cid, xs in LC.cases(key):
        want = from_fractions(q, xs)
        assert want is not None and LC.expected_ints(q, xs) == want, (key, cid)
        assert LC.signs(xs) == [lam < 0 for lam in exact(xs)], (key, cid)
        assert LC.expected_of(key, cid, xs) == b"".join(v.to_bytes(LC.HANDLES[key][1], "big") for v in want)
        assert all(0 <= v < q - 1 for v in want)


def test_the_big_case_against_exact_fractions_on_a_sample():
    xs, want = LC.big_expected()
    q = LC.modulus("b40")
    assert len(xs) == LC.BIG_M and sorted(xs) == list(range(1, LC.BIG_M + 1))
    whole = product(list(xs))
    for i in (0, 1, 15, 16, 255, 256, 257, 2048, 4080, 4095, 4096):
        diffs = [x - xs[i] for x in xs]
        del diffs[i]
        lam = Fraction(whole // xs[i], product(diffs))
        mag = abs(lam.numerator) * pow(lam.denominator, -1, (q - 1) // 2) % ((q - 1) // 2)
        v = mag if (lam > 0 or mag == 0) else (q - 1) - mag
        assert want[256 * i:256 * i + 256] == v.to_bytes(256, "big"), i


def test_the_fallback_lists():
    assert LC.expected_ints(23, LC.Q23_VALUE) == from_fractions(23, LC.Q23_VALUE) == [10, 12, 1]
    assert exact(LC.Q23_VALUE)[0] == Fraction(6, 5) and LC.raw_denominator_vanishes(LC.Q23_VALUE, 11)
    assert LC.expected_ints(23, LC.Q23_REFUSED) is None and from_fractions(23, LC.Q23_REFUSED) is None
    assert LC.expected_ints(23, LC.Q23_ON_DEVICE) == from_fractions(23, LC.Q23_ON_DEVICE) == [1, 0, 0]
    assert not LC.raw_denominator_vanishes(LC.Q23_ON_DEVICE, 11)
    assert LC.COMPOSITE_Q % 4 == 3 and LC.COMPOSITE_Q.bit_length() == 197 and K.H.width_for_bits(197) == LC.COMPOSITE_LPL
    for xs in LC.COMPOSITE_LISTS:
        assert LC.expected_ints(LC.COMPOSITE_Q, xs) == from_fractions(LC.COMPOSITE_Q, xs)
        assert not LC.raw_denominator_vanishes(xs, LC.COMPOSITE_SUB)


@pytest.mark.parametrize("key", ["q23", "b40", "b64"])
def test_the_exponents_reconstruct_what_the_reference_reconstructs(key):
    b = K.RtBuilder(key)
    q = b.q
    rng = random.Random(key)
    lists = [[3, 1, 2], [5, 2, 9, 4], LC.shape_positions(17)] if key != "q23" else [LC.Q23_VALUE, LC.Q23_ON_DEVICE, LC.Q23_REFUSED, [3, 4]]
    for xs in lists:
        shares = [pow(4, rng.randrange(1, b.sub), q) for _ in xs]
        ref = ref_reconstruct(b.G, xs, shares)
        exps = LC.expected_ints(q, xs)
        if exps is None:
            assert ref is REFUSED
            continue
        assert ref == math.prod(pow(s, e, q) for s, e in zip(shares, exps)) % q, (key, xs)
