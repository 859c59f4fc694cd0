"""Position lists and the reference for the Lagrange exponents of the run-time MODP groups on the device (k_rt_lagrange_terms,
k_rt_lagrange_finish; mpvss_modp_group_lagrange_exponents, mpvss_ctx_set_rt_lagrange).  tests/test_modp_rt_lagrange_cases.py holds
the reference to reconstruct_cases.exact_lagrange / ref_reconstruct on the CPU, tests/test_gpu_modp_rt_lagrange.py runs the kernels.

`expected` is Python integers only and depends on neither the engine nor the oracle: the exponent share i is raised to,
  mag = |num| den^-1 mod q', q' = (q-1)/2;   mag for a positive coefficient or mag = 0, (q - 1) - mag otherwise,
with num / den the coefficient as a fractions.Fraction in lowest terms where q' is below 2^64 (there a position or a difference of
two can share a factor with q', and the reference inverts the REDUCED denominator, participant.rs:546-553), and modular products with
pow(., -1, q') above (every factor is below 2^63 < q': a unit).  None: the reduced denominator has no inverse, the call refuses.

Sizes are the kernel's own edges.  A workgroup serves a TILE of 16 coefficients, one per DPP quad, and a list's positions pass
through LDS STAGE = 256 steps at a time (a list of m positions takes m - 1 steps per coefficient):
  1 (no step at all: the exponent is 1), 2, 3      the product loop at zero, one and two steps
  15, 16, 17                                       a tile short of one quad, full, and a second workgroup with one live quad
  255, 256, 257                                    STAGE - 1, STAGE and STAGE + 1 positions: 254, 255 and 256 steps, one staging trip
  513                                              2 STAGE + 1 positions: 512 steps, exactly two full trips
  258, 514                                         257 and 513 steps: a second and a third trip of one step
Position families: the shuffled 1..m of reconstruct_cases.Builder.shape_positions; 1..m ascending and descending (quad 0 of the
ascending list sees no negative difference, its last quad m - 1 of them, so both signs occur in every list of two or more); and the
int64 and 32-bit edges of reconstruct_cases.large_positions in its three orders.
Handles, one per width: 40 bits (5 limbs per lane), RFC 1024 (9), RFC 2048 (18), RFC 3526 group 15 (27) and group 16 (36); the
full ladder at the first three, WIDE_SIZES at the wide two, BIG_M = 4097 positions at 40 bits only."""
import math
import random

import modp_rt_4096_helpers as H4
import modp_rt_helpers as H
import modp_rt_reconstruct_cases as K
from reconstruct_cases import exact_lagrange, large_positions, orders

TILE = 16
STAGE = 256
DEVICE_MAX_M = 16384              # RT_LAGRANGE_DEVICE_MAX_M: a longer list keeps the host path
# key -> (modulus, bytes of an element on the ABI, limbs per lane the handle runs at)
HANDLES = {k: K.GROUPS[k] for k in ("b40", "rfc1024", "rfc2048", "rfc3072")}
HANDLES["rfc4096"] = (H4.group16, H4.EB, H4.LPL)
KEYS = tuple(HANDLES)
WIDE = ("rfc3072", "rfc4096")
SIZES = [1, 2, 3, TILE - 1, TILE, TILE + 1, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 1]
STEP_EDGE_SIZES = [STAGE + 2, 2 * STAGE + 2]
WIDE_SIZES = [1, 2, 3, 17, 65]
SPECIAL_M = {k: ([17] if k in WIDE else [8, 17, 65]) for k in KEYS}
BIG_M = 4097                      # at 40 bits: 257 workgroups, 17 staging trips
# the moduli of the fallback tests: q = 23 (q' = 11 divides positions and differences) and a composite q' of two Mersenne primes,
# where Fermat's power is no inverse
Q23 = 23
COMPOSITE_SUB = (2 ** 89 - 1) * (2 ** 107 - 1)
COMPOSITE_Q = 2 * COMPOSITE_SUB + 1
COMPOSITE_LPL = 5                 # 197 bits
Q23_VALUE = [1, 11, 12]           # raw denominators 0 mod 11, a value through the reduced fraction (132 / 110 = 6 / 5)
Q23_REFUSED = [1, 12]             # 12 / 11 and -1 / 11: no inverse even in lowest terms
Q23_ON_DEVICE = [11, 3, 1]        # every denominator a unit; two magnitudes 0 (11 in the numerator), one under a negative sign


def modulus(key):
    return HANDLES[key][0]()


def sizes(key):
    return WIDE_SIZES if key in WIDE else SIZES + STEP_EDGE_SIZES


def shape_positions(m):
    """reconstruct_cases.Builder.shape_positions without a builder (the same seed, the same list)"""
    xs = list(range(1, m + 1))
    random.Random(1000 + m).shuffle(xs)
    return xs


def cases(key):
    """[(id, positions)] of a handle"""
    out = []
    for m in sizes(key):
        out.append((f"shuffled-{m}", shape_positions(m)))
        if m > 1:
            out.append((f"asc-{m}", list(range(1, m + 1))))
            out.append((f"desc-{m}", list(range(m, 0, -1))))
    for m in SPECIAL_M[key]:
        for order, xs in orders(large_positions(m)).items():
            out.append((f"special-{m}-{order}", list(xs)))
    return out


def _product_mod(v, n):
    acc = 1
    for k in range(0, len(v), 16):
        acc = acc * math.prod(v[k:k + 16]) % n
    return acc


def denominators(positions):
    """[[|x_j - x_i| for j != i]]"""
    xs = list(positions)
    return [[abs(x - xi) for j, x in enumerate(xs) if j != i] for i, xi in enumerate(xs)]


def raw_denominator_vanishes(positions, sub):
    """some prod_{j != i} |x_j - x_i| shares a factor with q' before the fraction is reduced"""
    return any(math.gcd(_product_mod(d, sub), sub) != 1 for d in denominators(positions))


def signs(positions):
    """lambda_i < 0 exactly when an odd number of positions lie below x_i"""
    rank = {x: r for r, x in enumerate(sorted(positions))}
    return [rank[x] & 1 == 1 for x in positions]


def magnitudes(q, positions, units=False):
    """[|lambda_i| mod q'] or None where a reduced denominator has no inverse.  units: the caller knows every raw denominator to
    be a unit mod q' (big_expected), where num den^-1 is the value of the reduced fraction as it stands"""
    sub = (q - 1) // 2
    xs = list(positions)
    if len(set(xs)) != len(xs) or any(x < 1 for x in xs):
        raise ValueError("not a position list")
    if sub < 2 ** 64 and not units:
        out = []
        for lam in exact_lagrange(xs):
            try:
                out.append(abs(lam.numerator) * pow(lam.denominator, -1, sub) % sub)
            except ValueError:
                return None
        return out
    out = []
    for i, d in enumerate(denominators(xs)):
        num = _product_mod(xs[:i] + xs[i + 1:], sub)
        out.append(num * pow(_product_mod(d, sub), -1, sub) % sub)
    return out


def expected_ints(q, positions, units=False):
    """the m exponents, or None for a refusal"""
    mags = magnitudes(q, positions, units)
    if mags is None:
        return None
    return [mag if (not neg or mag == 0) else (q - 1) - mag for mag, neg in zip(mags, signs(positions))]


def expected(q, eb, positions):
    """the m exponents as eb big-endian bytes each, or None"""
    ints = expected_ints(q, positions)
    return None if ints is None else b"".join(v.to_bytes(eb, "big") for v in ints)


_MEMO = {}


def expected_of(key, cid, positions):
    """expected, computed once per (handle, case) of a test session"""
    if (key, cid) not in _MEMO:
        _MEMO[(key, cid)] = expected(modulus(key), HANDLES[key][1], positions)
    return _MEMO[(key, cid)]


def big_expected():
    """(positions, exponents as bytes) of the shuffled 1..BIG_M at 40 bits.  4097 exact fractions of 45 000-bit integers cost five
    seconds; here every factor, a position or a difference of two, lies in [1, BIG_M) and q' is a prime above that, so every raw
    denominator is a unit and the modular quotient is the reduced fraction's value (tests/test_modp_rt_lagrange_cases.py holds a
    sample of the coefficients to the exact fraction)."""
    if "big" not in _MEMO:
        q, xs = modulus("b40"), shape_positions(BIG_M)
        assert (q - 1) // 2 > BIG_M and H.miller_rabin((q - 1) // 2)
        _MEMO["big"] = (xs, b"".join(v.to_bytes(HANDLES["b40"][1], "big") for v in expected_ints(q, xs, units=True)))
    return _MEMO["big"]


# ---- the composite q' --------------------------------------------------------------------------------------------------------
# (a lone position is a case too: both accumulators stay at their start value R mod q', and Fermat's power does not invert that)
COMPOSITE_LISTS = [shape_positions(17), [5, 2, 9, 4], list(orders(large_positions(8))["shuffled"]), [7]]


def device_denominator(positions, i, sub, lpl):
    """what k_rt_lagrange_terms hands to Fermat's power for coefficient i: the product of the |x_j - x_i| times R = 2^(116 lpl),
    divided by 2^(29 lpl) once per step"""
    d = _product_mod(denominators(positions)[i], sub)
    return d * pow(2, 116 * lpl, sub) * pow(pow(2, 29 * lpl * (len(positions) - 1), sub), -1, sub) % sub


def check_composite():
    """Fermat's power inverts none of the denominators the composite cases use, as integers or as the device holds them: every one
    of these lists falls back to the host, which inverts them (they are units)"""
    sub = COMPOSITE_SUB
    for xs in COMPOSITE_LISTS:
        for i in range(len(xs)):
            d = _product_mod(denominators(xs)[i], sub)
            dd = device_denominator(xs, i, sub, COMPOSITE_LPL)
            assert math.gcd(d, sub) == 1
            assert (d == 1 or pow(d, sub - 1, sub) != 1) and pow(dd, sub - 1, sub) != 1, (xs, i)


check_composite()
