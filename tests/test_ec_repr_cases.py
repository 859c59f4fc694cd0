"""tests/ec_repr_cases.py held to its claims on the CPU: every limb vector stands for the value it is said to stand for and
lies in its class, every limb position of every coordinate is seen saturated and empty, and every scaled point is the point
the oracle says it is."""
import random

import pytest

import ec_repr_cases as R

pytestmark = pytest.mark.parametrize("name", R.NAMES)


def test_classes_and_their_union(name):
    u = R.CLASSES["U"][0]
    for cls in ("carried", "product", "mul_small"):
        bounds = R.CLASSES[cls][0]
        assert len(bounds) == R.NLIMB and all(b <= ub for b, ub in zip(bounds, u)), cls
    for i in range(R.NLIMB):                       # the union is tight: some class reaches U's bound in every limb but 0 and 1
        assert max(R.CLASSES[c][0][i] for c in ("carried", "product", "mul_small")) == (u[i] if i >= 2 else 2**27)


def test_representatives_stand_for_their_value_inside_their_class(name):
    p = R.PRIMES[name]
    rng = random.Random(len(name))
    values = [0, 1, 2, p - 1, p - 2, 2**255, 2**26 - 1, 2**26, (1 << 255) - 20] + [rng.randrange(p) for _ in range(200)]
    for cls in ("carried", "product", "mul_small", "U"):
        bounds = R.CLASSES[cls][0]
        for val in values:
            reps = R.representatives(val, p, bounds)
            assert reps[0] == ("canonical", R.limbs(val % p))
            assert "top-heavy" in [k for k, _ in reps]
            for kind, v in reps:
                assert R.value(v) % p == val % p and R.in_class(v, bounds), (cls, kind, hex(val))
            top = dict(reps)["top-heavy"]
            most = sum((b - 1) << (26 * i) for i, b in enumerate(bounds))
            assert most - p < R.value(top) <= most                              # no larger multiple of p fits
    reps = dict(R.representatives(values[-1] | 1 << 250, p, R.U))                # a full-width value: all four differ
    assert set(reps) == set(R.KINDS) and len({tuple(v) for v in reps.values()}) == 4
    # the top limb is within one p of its bound (p is 2^22 or 2^21 units of it), the low limb holds a unit of the one above
    assert R.U[9] - 1 - reps["top-heavy"][9] <= (p >> 234) + 1 and reps["bottom-heavy"][0] >= 2**26
    free = R.free_vectors(R.U)
    assert len(free) == 13 and all(R.in_class(v, R.U) and set(v) <= {0, R.U[0] - 1} for _, v in free)


def test_representatives_of_zero(name):
    p = R.PRIMES[name]
    zeros = R.zero_representatives(name)
    assert [t for t, _, _ in zeros] == ["p", "2 p, uncarried", "the subtraction pad", "the largest multiple of p in U, top-heavy"]
    for tag, v, cls in zeros:
        assert R.value(v) % p == 0 and R.value(v) != 0 and R.in_class(v, R.CLASSES[cls][0]), tag
    assert R.value(zeros[0][1]) == p and R.value(zeros[1][1]) == 2 * p
    assert not R.in_class(zeros[2][1], R.U)                                  # the pad is no stored coordinate's class


def test_every_limb_of_every_coordinate_is_seen_saturated_and_empty(name):
    rc = R.repr_cases(name)
    top = [b - 1 for b in R.U]
    for side in ("P", "Q"):
        for ci, c in enumerate(rc.coords):
            for i in range(R.NLIMB):
                seen = {getattr(case, side)[ci][i] for case in rc.cases}
                assert top[i] in seen and 0 in seen, (side, c, i)
    # the identity with every representative of zero in Z (secp256k1) / in X and in T (ristretto255), on either side
    for side, scalar in (("P", "a"), ("Q", "b")):
        ids = [getattr(case, side) for case in rc.cases if getattr(case, scalar) == 0]
        for _, z, _ in rc.zeros:
            for ci in ((2,) if name == "secp256k1" else (0, 3)):
                assert any(pt[ci] == z for pt in ids), (side, ci, z)
    kinds = {k for case in rc.cases for w in case.what for k in R.KINDS if k in w}
    assert kinds == set(R.KINDS)
    tags = {case.tag.split(";")[0] for case in rc.cases}
    assert {"a doubling", "P + (-P)", "the identity + Q", "P + the identity", "the identity twice"} <= tags
    assert 900 <= len(rc.cases) <= 4000


def test_every_written_point_is_the_point_it_claims_to_be(name):
    rc = R.repr_cases(name)
    e = rc.G.element_to_bytes
    for case in rc.cases:
        for vectors, k in ((case.P, case.a), (case.Q, case.b)):
            assert all(R.in_class(v, R.U) or v == rc.zeros[3][1] for v in vectors), case.tag
            assert e(rc.point_of(vectors)) == rc.enc(k), case.tag
    if name == "secp256k1":
        batches = rc.batches()
        assert {tag.split(",")[0] for tag, _ in batches} == {"identity in slot %d" % s for s in (0, 3, 4, 7)}
        for tag, row in batches:
            assert len(row) == 8 and sum(k == 0 for k, _ in row) == 1
            for k, vectors in row:
                assert e(rc.point_of(vectors)) == rc.enc(k), tag
                if k == 0:
                    assert any(vectors[2]) and R.value(vectors[2]) % rc.p == 0       # a non-zero zero
