"""CPU checks of the 4096-bit run-time MODP width (36 limbs per lane, L = 144, moduli of up to 4096 bits): an integer model of
bn::mont_mul (mpvss_rs_amd/csrc/bn_quad.h) WITH the second carry of a column that `if constexpr (K > 27)` adds -- in every row,
beside the retire step, the column at local position K / 2 moves its upper bits into the column at K / 2 + 1 and keeps its low
29 bits -- for the product, the squaring and the 144-row input product, with worst-case limbs and with random operands; the
constants of the width and RFC 3526 group 16; and the comb and twin models of tests/test_modp_rt_wide_model.py restated for
1 024 windows, with the operation counts DESIGN section 13 quotes for 4096 bits.  No GPU, no library.

Figures of the model (asserted below): without the second carry a column collects 2 x 36 = 72 products and passes 2^64; with it
a column holds at most 54 product units (a doubled limb of the squaring counts two) between two carries, 54 (2^29 + 511)^2 <
2^63.76, the bound of the 27-limb width; the plain product and the input product hold at most 38.  The carry-out of a lane in
the final pass stays below 2^37, as the comment at the end of bn::mont_mul says."""
import random

import pytest

import modp_rt_helpers as H
import modp_rt_4096_helpers as XH
import test_modp_rt_comb_model as CM
from test_modp_rt_model import LIMB_BOUND, M, W, limbs, val
from test_modp_rt_twin_model import twin_model

LPL, L, ROWS, TOP = XH.LPL, 4 * XH.LPL, 2 * XH.EB, XH.TOP
IN_ROWS = LPL * (-(-(-(-8 * XH.EB // W)) // LPL))          # LPL ceil(ceil(8 EB / 29) / LPL)
MID = LPL // 2                                              # the local position of the second carry
CAP = 29 * L - 2                                            # Width<36>::CAP_BITS


def mont_model36(a, b, N, rows, stats, square=False, bound_only=False, mid_carry=True):
    """bn::mont_mul<N0INV_RUNTIME, square, rows / 36> at K = 36 as integers, same step order: the products of the row, m, the
    products by the modulus, the second carry (position MID -> MID + 1), the retire step (position 0 -> 1, low bits to the lane
    below).  T[q K + k] is the column at local position k of lane q; the list shifts by one per row as the accumulators do.
    stats: maxacc, the largest accumulator; units, the most product units (a doubled limb counts two) a column collected between
    two carries; cout, the largest carry-out of a lane in the final pass.  mid_carry=False is the product as the narrower widths
    have it (to show that it overflows)."""
    lpl = LPL
    NL = limbs(N, L)
    n0inv = (-pow(N, -1, 1 << W)) % (1 << W)
    T, U = [0] * L, [0] * L
    for i in range(rows):
        bi = b[i]
        rr = i % lpl
        for j in range(L):
            k = j % lpl
            if not square:
                T[j] += a[j] * bi
                U[j] += 1
            elif k >= rr:
                T[j] += a[j] * (2 * bi if k > rr else bi)
                U[j] += 2 if k > rr else 1
        m = ((T[0] & 0xFFFFFFFF) * n0inv) & M
        for j in range(L):
            T[j] += m * NL[j]
            U[j] += 1
        assert T[0] & M == 0
        stats["maxacc"] = max(stats["maxacc"], max(T))
        stats["units"] = max(stats["units"], max(U))
        if mid_carry:
            for q in range(4):
                j = q * lpl + MID
                T[j + 1] += T[j] >> W
                T[j] &= M
                U[j] = 0
        for q in range(4):
            j = q * lpl
            T[j + 1] += T[j] >> W
            T[j] &= M
        stats["maxacc"] = max(stats["maxacc"], max(T))
        T = T[1:] + [0]
        U = U[1:] + [0]
        for q in range(4):
            U[q * lpl + lpl - 1] = 0                         # a lane's fresh top column: 29 bits from the lane above, or zero
    if bound_only:
        return None
    assert stats["maxacc"] < (1 << 64)
    out, couts = [0] * L, [0] * 4
    for q in range(4):
        c = 0
        for k in range(lpl):
            v = T[q * lpl + k] + c
            assert v < (1 << 64)
            out[q * lpl + k] = v & M
            c = v >> W
        couts[q] = c
    stats["cout"] = max(stats.get("cout", 0), max(couts))
    assert couts[3] == 0
    for q in range(1, 4):
        v = out[q * lpl] + couts[q - 1]
        out[q * lpl] = v & M
        out[q * lpl + 1] += v >> W
    return out


def new_stats():
    return {"maxacc": 0, "units": 0, "cout": 0}


def moduli(rng):
    return [XH.group16(), (1 << 4096) - 1, (1 << CAP) - 1, (1 << 3072) + 1, XH.odd_3073(), H.random_odd_modulus(4096, rng)]


def test_the_width_constants_and_group_16():
    assert (L, IN_ROWS, ROWS) == (144, 144, 1024)
    assert CAP == 4174 >= 4096 > 29 * 4 * 35 - 2, "R = 2^4176 > 4 N for every 4096-bit modulus; 35 limbs per lane would not do"
    assert MID == 18
    q = XH.group16()
    assert q.bit_length() == 4096 and q % 8 == 7
    assert H.miller_rabin(q, 2) and H.miller_rabin((q - 1) // 2, 2)
    assert XH.odd_3073().bit_length() == 3073 and XH.odd_3073() % 2 == 1


def test_without_the_second_carry_the_columns_overflow():
    """the product as the narrower widths have it: 72 product units in a column between two carries, product and squaring alike,
    which 64 bits do not bound (tests/test_modp_rt_wide_model.py::test_4096_bits_would_overflow_the_columns)"""
    for sq in (False, True):
        stats = new_stats()
        mont_model36([LIMB_BOUND] * L, [LIMB_BOUND] * L, (1 << CAP) - 1, L, stats, square=sq, bound_only=True, mid_carry=False)
        assert stats["units"] == 2 * LPL == 72
    assert 72 * LIMB_BOUND * LIMB_BOUND >= 1 << 64


@pytest.mark.parametrize("N", [(1 << CAP) - 1, XH.group16()], ids=["2^4174-1", "group16"])
def test_worst_case_limbs_stay_below_2_64_with_the_second_carry(N):
    """every limb at the almost-normalised bound (far above 2N as an integer).  The plain product and the 144-row input
    product: a column collects 2 x 18 = 36 products above the middle and 36 below it, plus what the carries bring -- at most 38
    product units' worth.  The squaring puts its doubled limbs into a column unevenly over the column's life: the column that
    enters a lane in row 0 takes a doubled product in each of its first 18 rows (36 units) beside 18 products by the modulus,
    54 units before the second carry and 18 after -- the 27-limb width's bound, 54 (2^29 + 511)^2 < 2^63.76."""
    unit = LIMB_BOUND * LIMB_BOUND
    assert 54 * unit + (1 << 40) < 1 << 64
    for kind, args, units, bound in (
        ("product", dict(b=[LIMB_BOUND] * L, rows=L), 36, 38 * unit),
        ("squaring", dict(b=[LIMB_BOUND] * L, rows=L, square=True), 54, 54 * unit + (1 << 40)),
        ("input product", dict(b=[M] * IN_ROWS, rows=IN_ROWS), 36, 38 * unit),
    ):
        stats = new_stats()
        mont_model36([LIMB_BOUND] * L, N=N, stats=stats, bound_only=True, **args)
        assert stats["units"] == units, kind
        assert stats["maxacc"] < bound < 1 << 64, kind


def test_product_and_squaring_match_montgomery_at_36_limbs_per_lane():
    rng = random.Random(36)
    R = 1 << (W * L)
    stats = new_stats()
    n0invs = set()
    for N in moduli(rng):
        assert 4 * N < R
        n0invs.add((-pow(N, -1, 1 << W)) % (1 << W))
        rinv = pow(R, -1, N)
        cases = [(2 * N - 1, 2 * N - 1), (0, 2 * N - 1), (1, N)] + [(rng.randrange(2 * N), rng.randrange(2 * N)) for _ in range(3)]
        for a, b in cases:
            for sq in (False, True):
                bb = a if sq else b
                r = mont_model36(limbs(a, L), limbs(bb, L), N, L, stats, square=sq)
                v = val(r)
                assert v < 2 * N and v % N == a * bb * rinv % N
                assert max(r) <= LIMB_BOUND
    assert len(n0invs - {1}) >= 2, "the run-time n0inv must be exercised with values other than 1"
    assert stats["maxacc"] < (1 << 64)
    assert stats["cout"] < 1 << 37, "the carry-out of a lane in the final pass (bn::mont_mul, pass 2)"


def test_almost_normalised_operands_give_the_same_product():
    """operands whose limbs carry the slack a previous product may leave (every limb up to 2^29 - 1 + 2^9, value < 2N)"""
    rng = random.Random(3636)
    R = 1 << (W * L)
    stats = new_stats()
    for N in (XH.group16(), XH.odd_3073()):
        rinv = pow(R, -1, N)
        for sq in (False, True):
            a = rng.randrange(N)
            b = a if sq else rng.randrange(N)
            la, lb = limbs(a, L), limbs(b, L)
            for l in ((la,) if sq else (la, lb)):
                for j in range(0, L - 1, 3):                  # move 2^29 from limb j + 1 down into limb j where the bound allows
                    if l[j + 1] > 0 and l[j] <= 511:
                        l[j + 1] -= 1
                        l[j] += 1 << W
            assert val(la) == a and max(la) <= LIMB_BOUND
            r = mont_model36(la, la if sq else lb, N, L, stats, square=sq)
            v = val(r)
            assert v < 2 * N and v % N == a * b * rinv % N and max(r) <= LIMB_BOUND


def test_the_input_product_brings_any_512_byte_value_into_the_width():
    """to_mont_in at 36 limbs per lane: IN_ROWS = L, so kin = R^2 mod N and the product is a plain 4-group one; x R mod N below
    2N for inputs up to 2^4096 - 1"""
    rng = random.Random(436)
    R = 1 << (W * L)
    stats = new_stats()
    for N in moduli(rng):
        kin = pow(2, W * (IN_ROWS + L), N)
        assert kin == R * R % N
        for x in (0, N, N + 1, TOP, rng.randrange(1 << 4096), rng.randrange(N)):
            r = mont_model36(limbs(kin, L), limbs(x, IN_ROWS), N, IN_ROWS, stats)
            v = val(r)
            assert v < 2 * N and v % N == x * R % N
            assert max(r) <= LIMB_BOUND
    assert stats["maxacc"] < (1 << 64) and stats["cout"] < 1 << 37


# ---- the comb and twin models at 1 024 windows -----------------------------------------------------------------------
class Lazy36(CM.Lazy):
    """CM.Lazy at 36 limbs per lane: R = 2^(29 x 144), the input product of 144 rows"""

    def __init__(self, q):
        self.q, self.lpl, self.L = q, LPL, L
        self.rbits = 29 * L
        self.R = 1 << self.rbits
        assert self.R > 4 * q
        self.ninv = (-pow(q, -1, self.R)) % self.R
        self.one_m = self.R % q
        self.in_bits = 29 * IN_ROWS
        self.kin = pow(2, self.in_bits + self.rbits, q)
        self.ops = {"entry": 0, "build": 0, "table": 0, "square": 0, "window": 0, "comb": 0, "exit": 0}

    def to_mont_in(self, x):
        assert 0 <= x <= TOP
        self.ops["entry"] += 1
        t = x * self.kin
        t = (t + ((t * self.ninv) & (self.R - 1)) * self.q) >> self.in_bits      # IN_ROWS = L: the same R
        assert t < 2 * self.q and t % self.q == x * self.R % self.q
        return t


def comb_build(m, base):
    """k_rt_comb_bases and k_rt_comb_rows with 1 024 rows"""
    comb = [[m.one_m] + [0] * 15 for _ in range(ROWS)]
    acc = m.to_mont_in(base)
    for k in range(ROWS):
        comb[k][1] = acc
        if k + 1 < ROWS:
            for _ in range(4):
                acc = m.mul(acc, acc, "build")
    for k in range(ROWS):
        acc = comb[k][1]
        for d in range(2, 16):
            acc = m.mul(acc, comb[k][1], "build")
            comb[k][d] = acc
    return comb


def comb_exp_wave(m, comb, E1):
    """phase B of k_rt_comb_exp (g^e alone) over 1 024 rows"""
    n = len(E1)
    assert 1 <= n <= 16 and all(0 <= e <= TOP for e in E1)
    acc = [m.one_m] * n
    nw1 = (max(e.bit_length() for e in E1) + 3) // 4
    assert nw1 <= ROWS
    for k in range(nw1):
        if all(CM.nib(e, k) == 0 for e in E1):
            continue
        acc = m.wave_mul(acc, [comb[k][CM.nib(e, k)] for e in E1], "comb")
    return [m.canonical(a) for a in m.wave_mul(acc, [1] * n, "exit")]


def left_to_right(m, base, e):
    """k_rt_table + k_rt_dual_exp for one exponent"""
    tab = CM.table16(m, base)
    nw = (e.bit_length() + 3) // 4
    acc = tab[CM.nib(e, nw - 1)] if nw else m.one_m
    for w in range(nw - 2, -1, -1):
        for _ in range(4):
            acc = m.mul(acc, acc, "square")
        acc = m.mul(acc, tab[CM.nib(e, w)], "window")
    return m.canonical(m.mul(acc, 1, "exit"))


@pytest.fixture(scope="module")
def comb16():
    m = Lazy36(XH.group16())
    return m, comb_build(m, 4)


def test_lazy_product_is_the_limb_level_product_at_36():
    rng = random.Random(5)
    q = XH.group16()
    m = Lazy36(q)
    for sq in (False, True):
        a = rng.randrange(2 * q)
        b = a if sq else rng.randrange(2 * q)
        want = val(mont_model36(limbs(a, L), limbs(b, L), q, L, new_stats(), square=sq))
        assert m.mul(a, b) == want


def test_comb_model_equals_pow_at_1024_windows(comb16):
    m, comb = comb16
    q = m.q
    assert m.ops["build"] == 4 * (ROWS - 1) + 14 * ROWS == 4092 + 14336
    assert all(comb[k][d] % q == pow(4, d << (4 * k), q) * m.R % q for k in (0, 1, 767, 768, 1023) for d in range(16))
    rng = random.Random(16)
    edge = [0, 1, 15, 16, 1 << 4095, TOP, q - 1, q - 2, 1 << 3072]
    while len(edge) < 16:
        edge.append(rng.randrange(1 << 4096))
    top_only = [rng.randrange(1, 16) << (4 * (ROWS - 1))] + [0] * 15
    for E in (edge, top_only, [0], [5, rng.getrandbits(4096) | (1 << 4095), rng.getrandbits(64)]):
        assert comb_exp_wave(m, comb, E) == [pow(4, e, q) for e in E]


def test_operation_counts_at_4096_bits(comb16):
    m, comb = comb16
    q = m.q
    before = dict(m.ops)
    assert comb_exp_wave(m, comb, [TOP] * 16) == [pow(4, TOP, q)] * 16
    fixed = {k: m.ops[k] - before[k] for k in m.ops}
    assert fixed == {"entry": 0, "build": 0, "table": 0, "square": 0, "window": 0, "comb": 1024, "exit": 1}
    assert sum(fixed.values()) == 1025
    m2 = Lazy36(q)
    assert left_to_right(m2, 4, TOP) == pow(4, TOP, q)
    assert m2.ops == {"entry": 1, "build": 0, "table": 14, "square": 4092, "window": 1023, "comb": 0, "exit": 1}
    assert sum(m2.ops.values()) == 5131
    r1, r2, ops = twin_model(q, L, 3, TOP, TOP)
    assert (r1, r2) == (pow(3, TOP, q),) * 2
    assert ops == {"entry": 1, "square": 4092, "bucket": 2048, "combine": 56, "exit": 2}
    assert sum(ops.values()) == 6199


def test_twin_model_equals_pow_at_4096_bits():
    rng = random.Random(41)
    q = XH.group16()
    for e1, e2 in [(0, TOP), (1 << 3072, 3), (rng.getrandbits(4096), rng.getrandbits(3073))]:
        for base in (0, q - 1, q + 1, TOP, rng.getrandbits(4096)):
            r1, r2, _ = twin_model(q, L, base, e1, e2)
            assert (r1, r2) == (pow(base, e1, q), pow(base, e2, q))
