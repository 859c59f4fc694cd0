"""Position lists and the reference for the Lagrange coefficients of the curve groups (k_ec_lagrange; mpvss_ec_lagrange_scalars,
mpvss_ctx_set_ec_lagrange).  tests/test_ec_lagrange_cases.py holds the reference to reconstruct_cases.exact_lagrange on the CPU,
tests/test_ec_lagrange_host_unit.py runs the kernel's lane body on the CPU against it, tests/test_gpu_ec_lagrange.py the kernel.

`expected` is Python integers only: (prod_{j != i} x_j) (prod_{j != i} (x_j - x_i))^-1 mod the order, in the group's scalar byte
order.  It depends on neither the engine nor the oracle.

Sizes are the kernel's own edges.  A workgroup is WG = 64 lanes, one coefficient each, and a list's positions pass through LDS
STAGE = 256 at a time:
  1 (lambda = 1: no factor at all), 2, 3          the product loops at zero, one and two steps
  63, 64, 65                                       a tile short of one lane, full, and a second workgroup with one live lane
  255, 256, 257                                    the staging tile short of one position, full, and a second trip of one
  513                                              two staging tiles and one position: the lane's own index skipped in tile 0, 1 or 2
Position families: the shuffled 1..m of reconstruct_cases.Builder.shape_positions; 1..m ascending and descending (lane 0 of the
ascending list sees no negative difference, its last lane m - 1 of them, so both parities of the sign occur in every list of two or
more); and the int64 and 32-bit edges of reconstruct_cases.SPECIAL in three orders at m = 8, 17 and 65."""
import math
import random

from reconstruct_cases import large_positions, orders

WG = 64
STAGE = 256
ORDER = {
    "secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
    "ristretto255": 2 ** 252 + 27742317777372353535851937790883648493,
}
BYTE_ORDER = {"secp256k1": "big", "ristretto255": "little"}
CURVES = tuple(ORDER)
SIZES = [1, 2, 3, WG - 1, WG, WG + 1, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 1]
SPECIAL_M = [8, 17, 65]
BIG_M = 4097                      # reconstruct_cases.SHAPE_M_BIG's odd size: 65 workgroups, 17 staging trips


def shape_positions(m):
    """reconstruct_cases.Builder.shape_positions without a builder (the same seed, the same list)"""
    xs = list(range(1, m + 1))
    random.Random(1000 + m).shuffle(xs)
    return xs


def cases():
    """[(id, positions)]"""
    out = []
    for m in SIZES:
        out.append((f"shuffled-{m}", shape_positions(m)))
        out.append((f"asc-{m}", list(range(1, m + 1))))
        out.append((f"desc-{m}", list(range(m, 0, -1))))
    for m in SPECIAL_M:
        for order, xs in orders(large_positions(m)).items():
            out.append((f"special-{m}-{order}", list(xs)))
    return out


def _product_mod(v, n):
    """the product of the integers v, reduced mod n (the residue of the exact product: the exact integer of 4096 factors costs a
    thousand times the reduced one)"""
    acc = 1
    for k in range(0, len(v), 16):
        acc = acc * math.prod(v[k:k + 16]) % n
    return acc


def expected_ints(name, positions):
    """[(prod_{j != i} x_j) (prod_{j != i} (x_j - x_i))^-1 mod n]"""
    n = ORDER[name]
    xs = list(positions)
    out = []
    for i, xi in enumerate(xs):
        diffs = [x - xi for x in xs]
        del diffs[i]
        num = _product_mod(xs[:i] + xs[i + 1:], n)
        out.append(num * pow(_product_mod(diffs, n), -1, n) % n)
    return out


def expected(name, positions):
    """the m scalars as bytes, 32 each in the group's scalar byte order"""
    return b"".join(v.to_bytes(32, BYTE_ORDER[name]) for v in expected_ints(name, positions))


_MEMO = {}


def expected_of(name, cid, positions):
    """expected, computed once per (curve, case) of a test session"""
    key = (name, cid)
    if key not in _MEMO:
        _MEMO[key] = expected(name, positions)
    return _MEMO[key]
