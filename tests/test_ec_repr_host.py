"""The curve kernels' field and one-lane point arithmetic on WEAKLY REDUCED operands, on the CPU: ec_field.h / ec_curves.h
compiled with g++ (tests/ec_host_shim.cpp), every operation driven at the limb bounds it states -- and, where the header
stated none or one its callers exceed, at the bound derived below -- against Python integers; the point formulas on the
cases of tests/ec_repr_cases.py (saturated limbs in every position of every coordinate, non-canonical identities) against
the canonical encodings of oracle/ec_ref.c.

Derived bounds (ec_field.h states them since this test exists):
  mul_small  any u32 limbs, k < 2^6: the chain runs in 64 bits, x < 2^38 + 2^12, so t < 2^12 + 1 and t R0 < 2^26.
             Largest caller: OctSecp::add, x = A + (pad - B) + (pad - C) <= (2^27 + 2^12 - 1) + 2 (2^29 - 8) > 2^30, K <= 21.
  sub / neg  b[i] <= subpad(i) (no limb goes below zero) and a[i] + subpad(i) - b[i] < 2^31 (carry's input bound).
  mul2       the folds add less than 2^43 to a column (pieces < 2^26, R0 < 2^14, R1 <= 2^10, at most six of them and the
             wrap-around), a column holds at most 10 products of each pair, so A B + C D <= (2^64 - 2^43) / 10 for the
             limb bounds A, B, C, D of the four factors; QuadSecp::add's largest pair is
             (2^27 + 2^29)(2^28) + (2^27)(2^27) ~ 2^57.4."""
import ctypes as C
import math
import random
import time

import pytest

import ec_dual_cases
import ec_repr_cases as R

CURVES = [(0, "secp256k1"), (1, "ristretto255")]
ZERO = [0] * 10
U_TOP = R.U[0] - 1
CARRY_IN = 2**31 - 1                              # ec_field.h, carry: 'limbs in: < 2^31'
HEADER_SUB = 2**29 - 2**26 - 1                    # ec_field.h, sub, as it read before: 'b limbs < 2^29 - 2^26'
SMALL_CLASS = R.CLASSES["mul_small"][0]


@pytest.fixture(scope="module")
def shim():
    lib = ec_dual_cases.load_shim()
    lib.fe_repr_op.restype = C.c_uint32
    return lib


def arr(v):
    return (C.c_uint32 * len(v))(*v)


def fe(shim, curve, op, a, b=ZERO, c=ZERO, d=ZERO, k=0):
    """-> (return value, the limbs the operation left, the value of its canonical bytes)"""
    out, lim = (C.c_uint8 * 32)(), (C.c_uint32 * 10)()
    ret = shim.fe_repr_op(curve, op, arr(a), arr(b), arr(c), arr(d), k, lim, out)
    return ret, list(lim), int.from_bytes(bytes(out), "little")


def patterns(rng, top, count=300):
    """worst-case and seeded random limb patterns up to the inclusive per-limb bound `top`"""
    out = [list(top), [t - 1 for t in top], [t if i % 2 == 0 else 0 for i, t in enumerate(top)],
           [t if i % 2 == 1 else 0 for i, t in enumerate(top)]]
    out += [[t if i == k else 0 for i, t in enumerate(top)] for k in range(10)]
    out += [[rng.randrange(t + 1) for t in top] for _ in range(count)]
    out += [[rng.choice((0, t, t - 1, t // 2)) for t in top] for _ in range(count // 2)]
    return out


@pytest.mark.parametrize("curve,name", CURVES)
def test_carry_and_addc_over_their_whole_input_domain(shim, curve, name):
    """limbs (for addc: sums of limbs) up to 2^31 - 1 -> the value, in the carried class"""
    p, rng, carried = R.PRIMES[name], random.Random(31 + curve), R.CLASSES["carried"][0]
    for s in patterns(rng, [CARRY_IN] * 10):
        _, lim, got = fe(shim, curve, 4, s)
        assert got == R.value(s) % p and R.in_class(lim, carried), s
        a = [rng.randrange(x + 1) for x in s]
        b = [x - y for x, y in zip(s, a)]
        for op in (2, 3):                         # add then carry, addc
            _, lim, got = fe(shim, curve, op, a, b)
            assert got == R.value(s) % p and R.in_class(lim, carried), (op, a, b)


@pytest.mark.parametrize("curve,name", CURVES)
def test_sub_and_neg_at_the_pad(shim, curve, name):
    """subtrahend limbs up to 2^29 - 2^26 - 1 (the header's old wording), then up to subpad(i) itself; the minuend up to
    the largest that keeps a + pad - b below 2^31 -> the value, in the carried class"""
    p, rng, carried = R.PRIMES[name], random.Random(29 + curve), R.CLASSES["carried"][0]
    pad = R.header_table(name, "subpad")
    assert R.value(pad) % p == 0 and all(HEADER_SUB < x < 2**29 for x in pad)
    for btop in ([HEADER_SUB] * 10, pad):
        for it, b in enumerate(patterns(rng, btop, 200)):
            _, lim, got = fe(shim, curve, 1, b)
            assert got == -R.value(b) % p and R.in_class(lim, carried), b
            atop = [CARRY_IN - x + y for x, y in zip(pad, b)]
            for a in (atop, ZERO, [rng.randrange(t + 1) for t in atop], [rng.choice((0, t, t - 1, U_TOP)) for t in atop]):
                _, lim, got = fe(shim, curve, 0, a, b)
                assert got == (R.value(a) - R.value(b)) % p and R.in_class(lim, carried), (a, b)


@pytest.mark.parametrize("curve,name", CURVES)
def test_mul_small_at_and_beyond_its_largest_caller(shim, curve, name):
    """k in {1, 3, 21, 63}; limbs up to what OctSecp::add feeds (above 2^30), then any 32-bit limbs -> the value, inside
    the class ec_field.h states for the result"""
    p, rng = R.PRIMES[name], random.Random(63 + curve)
    caller = U_TOP + 2 * max(R.header_table("secp256k1", "subpad"))
    assert 2**30 < caller < 2**31
    for top in (caller, 2**32 - 1):
        for a in patterns(rng, [top] * 10, 200):
            for k in (1, 3, 21, 63):
                _, lim, got = fe(shim, curve, 5, a, k=k)
                assert got == R.value(a) * k % p and R.in_class(lim, SMALL_CLASS), (a, k)


def mul2_bounds(name):
    """[(tag, (A, B, C, D) inclusive per-limb bounds)]"""
    pad = R.header_table(name, "subpad")
    small = [b - 1 for b in SMALL_CLASS]                              # m, crk: results of mul_small
    mm = [s + q for s, q in zip(small, pad)]                          # m + pad - m': no carry
    zz = [2 * s for s in small]                                       # m + m': no carry
    assert max(mm) < 2**30 and max(pad) < 2**30                       # ec_quad.h: 'a factor of mul2: no carry, < 2^30'
    budget = (2**64 - 2**43) // 10
    even = math.isqrt(budget // 2)
    rest = math.isqrt(budget - (2**30 - 1)**2)
    assert 2 * even * even <= budget < 2 * (even + 1)**2 and (2**30 - 1)**2 + rest * rest <= budget
    hdr = int(2**28.5)
    return [("the header's old 2^28.5 on all four", ([hdr] * 10,) * 4),
            ("QuadSecp::add lane 0: crk mm' + crk' (-crk'')", (small, mm, small, pad)),
            ("QuadSecp::add lane 1: mm zz + crk m", (mm, zz, small, small)),
            ("QuadSecp::add lane 2: zz crk + m crk", (zz, small, small, small)),
            ("derived: four equal factors, A B + C D at the budget", ([even] * 10,) * 4),
            ("derived: one pair at mul's 2^30 - 1, the other takes the rest", ([2**30 - 1] * 10, [2**30 - 1] * 10, [rest] * 10, [rest] * 10))]


@pytest.mark.parametrize("curve,name", CURVES)
def test_mul2_at_the_header_bound_at_its_callers_and_at_the_derived_bound(shim, curve, name):
    p, rng, product = R.PRIMES[name], random.Random(57 + curve), R.CLASSES["product"][0]
    for tag, tops in mul2_bounds(name):
        pats = [patterns(rng, t, 100) for t in tops]
        for it in range(len(pats[0])):
            a, b, c, d = pats[0][it], pats[1][(it * 7 + 3) % len(pats[1])], pats[2][(it * 5 + 1) % len(pats[2])], pats[3][(it * 3 + 2) % len(pats[3])]
            if it < 2:
                b, c, d = pats[1][it], pats[2][it], pats[3][it]       # all four at the bound, at the bound - 1
            _, lim, got = fe(shim, curve, 6, a, b, c, d)
            assert got == (R.value(a) * R.value(b) + R.value(c) * R.value(d)) % p and R.in_class(lim, product), (tag, a, b, c, d)


@pytest.mark.parametrize("curve,name", CURVES)
def test_canon_and_the_predicates_on_every_representative(shim, curve, name):
    """canon, is_zero, is_odd over carry's whole input domain and equal over sub's: every representative of 0, 1, p - 1
    and of random values -> the canonical limbs and bytes / the boolean Python gives"""
    p, rng = R.PRIMES[name], random.Random(11 + curve)
    pad = R.header_table(name, "subpad")
    wide = [CARRY_IN + 1] * 10
    targets = [0, 1, p - 1, 2, p - 2, (p - 1) // 2, (p + 1) // 2] + [rng.randrange(p) for _ in range(40)]
    vectors = [v for _, v, _ in R.zero_representatives(name)]
    for val in targets:
        for bounds in (R.U, wide, R.CLASSES["carried"][0], R.CLASSES["product"][0]):
            vectors += [v for _, v in R.representatives(val, p, bounds)]
        for _ in range(6):                        # random limbs plus what is missing to the target, uncarried
            r = [rng.randrange(2**30) for _ in range(10)]
            vectors.append([x + y for x, y in zip(r, R.limbs((val - R.value(r)) % p))])
    vectors += patterns(rng, [CARRY_IN] * 10, 200)
    zeros = 0
    for v in vectors:
        assert R.in_class(v, wide)
        want = R.value(v) % p
        _, lim, got = fe(shim, curve, 7, v)
        assert lim == R.limbs(want) and got == want, v
        assert fe(shim, curve, 8, v)[0] == (want == 0), v
        assert fe(shim, curve, 10, v)[0] == want % 2, v
        zeros += want == 0
    assert zeros >= 4 + 6 + 8                     # the named ones, the random ones, representatives(0) in the classes
    # equal(a, b) = is_zero(a - b): b within the pad, a within what sub leaves room for
    btop, atop = [x + 1 for x in pad], [CARRY_IN + 1 - x for x in pad]
    for val in targets:
        bs = [v for _, v in R.representatives(val, p, btop) + R.representatives(val, p, R.U)]
        for other in (val, val + 1, val - 1, p - val, rng.randrange(p)):
            for _, a in R.representatives(other, p, atop) + R.representatives(other, p, R.U):
                for b in bs:
                    assert fe(shim, curve, 9, a, b)[0] == ((other - val) % p == 0), (a, b)


# ---- the one-lane point formulas ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,name", CURVES)
def test_point_formulas_on_weak_operands(shim, curve, name):
    """add, dbl, neg, add_affine and add_cached with both signs, cmov, encode, ks_is_identity and 64 steps of acc += Q /
    acc = 2 acc on every case of ec_repr_cases: byte for byte the oracle's encodings"""
    t0 = time.time()
    rc = R.repr_cases(name)
    t1 = time.time()
    out = (C.c_uint8 * (11 * rc.L))()
    for case in rc.cases:
        assert shim.ec_repr_pair(curve, arr([x for v in case.P for x in v]), arr([x for v in case.Q for x in v]), out) == 11
        got = bytes(out)
        for s, want in enumerate(R.expected_slots(rc, case)):
            assert got[s * rc.L:(s + 1) * rc.L] == want, (R.SLOT_NAMES[s], case.tag)
    print("%s: %d cases, building them %.1f s (the oracle's part included), running them %.1f s" % (name, len(rc.cases), t1 - t0, time.time() - t1))


def test_secp256k1_batched_encoding_with_weak_and_vanishing_z(shim):
    """encode_batch<8>: a weak-Z point, an identity written with a non-zero zero (first, last, in the middle) and ordinary
    points share one inversion"""
    rc = R.repr_cases("secp256k1")
    out = (C.c_uint8 * (8 * 33))()
    for tag, row in rc.batches():
        assert shim.secp_repr_batch8(arr([x for _, pt in row for v in pt for x in v]), out) == 0
        assert bytes(out) == b"".join(rc.enc(k) for k, _ in row), tag
