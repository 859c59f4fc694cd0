"""CPU checks of the wide run-time MODP width (27 limbs per lane, L = 108, moduli of up to 3072 bits): the integer model of
bn::mont_mul of tests/test_modp_rt_model.py at lpl = 27 -- product, squaring and the 108-row product that takes a 384-byte
input -- with the column bound for worst-case limbs; the analytic count that excludes 4096 bits; and the comb and twin models
of tests/test_modp_rt_comb_model.py / test_modp_rt_twin_model.py restated for 768 windows, with the operation counts DESIGN
section 13 quotes for 3072 bits.  No GPU, no library."""
import random

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import test_modp_rt_comb_model as CM
import test_modp_rt_model as LM
from test_modp_rt_twin_model import twin_model

LPL, L, ROWS, TOP = WH.LPL, 4 * WH.LPL, 2 * WH.EB, WH.TOP
W = LM.W
IN_ROWS = LPL * (-(-(-(-8 * WH.EB // W)) // LPL))          # LPL ceil(ceil(8 EB / 29) / LPL)


def wide_moduli(rng):
    return [WH.group15(), (1 << 3072) - 1, (1 << 2048) + 1, H.random_odd_modulus(2049, rng), H.random_odd_modulus(3072, rng)]


def test_the_wide_width_constants():
    assert (L, IN_ROWS, ROWS) == (108, 108, 768)
    assert 29 * L - 2 == 3130 >= 3072, "R = 2^(29 L) > 4 N for every 3072-bit modulus"
    q = WH.group15()
    assert q.bit_length() == 3072 and q % 8 == 7
    assert H.miller_rabin(q, 4) and H.miller_rabin((q - 1) // 2, 4)


def test_product_and_squaring_match_montgomery_at_27_limbs_per_lane():
    rng = random.Random(27)
    R = 1 << (W * L)
    stats = {"maxacc": 0}
    n0invs = set()
    for N in wide_moduli(rng):
        assert 4 * N < R
        n0invs.add((-pow(N, -1, 1 << W)) % (1 << W))
        rinv = pow(R, -1, N)
        cases = [(2 * N - 1, 2 * N - 1), (0, 2 * N - 1), (1, N)] + [(rng.randrange(2 * N), rng.randrange(2 * N)) for _ in range(3)]
        for a, b in cases:
            for sq in (False, True):
                bb = a if sq else b
                r = LM.mont_model(LM.limbs(a, L), LM.limbs(bb, L), N, LPL, L, stats, square=sq)
                v = LM.val(r)
                assert v < 2 * N and v % N == a * bb * rinv % N
                assert max(r) <= LM.LIMB_BOUND
    assert len(n0invs - {1}) >= 2, "the run-time n0inv must be exercised with values other than 1"
    assert stats["maxacc"] < (1 << 64)


def test_worst_case_limbs_stay_below_2_64():
    """every limb at the almost-normalised bound, product, squaring and the 108-row input product: at most 2 x 27 = 54
    products between two carries of a column, 54 (2^29 - 1 + 2^9)^2 + carry < 2^64"""
    assert 2 * LPL * LM.LIMB_BOUND ** 2 + (1 << 40) < 1 << 64
    for N in ((1 << 3130) - 1, WH.group15()):
        stats = {"maxacc": 0}
        LM.mont_model([LM.LIMB_BOUND] * L, [LM.LIMB_BOUND] * L, N, LPL, L, stats, bound_only=True)
        LM.mont_model([LM.LIMB_BOUND] * L, [LM.LIMB_BOUND] * L, N, LPL, L, stats, square=True, bound_only=True)
        LM.mont_model([LM.LIMB_BOUND] * L, [LM.M] * IN_ROWS, N, LPL, IN_ROWS, stats, bound_only=True)
        assert stats["maxacc"] < 2 * LPL * LM.LIMB_BOUND ** 2 + (1 << 40)


def test_the_input_product_brings_any_384_byte_value_into_the_width():
    """to_mont_in at the wide width: IN_ROWS = L, so kin = R^2 mod N and the product is a plain 4-group one; x R mod N below
    2N for inputs up to 2^3072 - 1"""
    rng = random.Random(227)
    R = 1 << (W * L)
    stats = {"maxacc": 0}
    for N in wide_moduli(rng):
        kin = pow(2, W * (IN_ROWS + L), N)
        assert kin == R * R % N
        for x in (0, N, N + 1, TOP, rng.randrange(1 << 3072), rng.randrange(N)):
            r = LM.mont_model(LM.limbs(kin, L), LM.limbs(x, IN_ROWS), N, LPL, IN_ROWS, stats)
            v = LM.val(r)
            assert v < 2 * N and v % N == x * R % N
            assert max(r) <= LM.LIMB_BOUND
    assert stats["maxacc"] < (1 << 64)


def test_4096_bits_would_overflow_the_columns():
    """36 limbs per lane (L = 144, 4174 bits) is the next width: a column then collects 72 products between two carries, and
    72 (2^29 + 511)^2 >= 2^64 -- so 4096-bit groups need a carry in the middle of a group of rows and are not offered"""
    assert 29 * 4 * 36 - 2 >= 4096 > 29 * 4 * 35 - 2
    assert 2 * 36 * ((1 << 29) + 511) ** 2 >= 1 << 64
    assert 2 * 27 * ((1 << 29) + 511) ** 2 + (1 << 36) < 1 << 64


# ---- the comb and twin models at 768 windows -------------------------------------------------------------------------
class LazyWide(CM.Lazy):
    """CM.Lazy at 27 limbs per lane: R = 2^(29 x 108), the input product of 108 rows"""

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


def comb_build(m, base, mutant=None):
    """CM.comb_build with 768 rows"""
    comb = [[m.one_m] + [0] * 15 for _ in range(ROWS)]
    acc = m.to_mont_in(base)
    for k in range(ROWS):
        comb[k][1] = acc
        if k + 1 < ROWS:
            for _ in range(3 if mutant == "row base ^8" else 4):
                acc = m.mul(acc, acc, "build")
    for k in range(ROWS):
        acc = comb[k][1]
        for d in range(2, 16):
            acc = m.mul(acc, comb[k][1], "build")
            comb[k][d + 1 if mutant == "entry d off by one" and d < 15 else d] = acc
    return comb


def comb_exp_wave(m, comb, E1, mutant=None):
    """phase B of CM.comb_exp_wave (g^e alone) over 768 rows"""
    n = len(E1)
    assert 1 <= n <= 16 and all(0 <= e <= TOP for e in E1)
    acc = [m.one_m] * n
    nw1 = (max(e.bit_length() for e in E1) + 3) // 4
    assert nw1 <= ROWS
    for k in range(1 if mutant == "phase B from k = 1" else 0, nw1):
        if all(CM.nib(e, k) == 0 for e in E1):
            continue
        acc = m.wave_mul(acc, [comb[k][CM.nib(e, k)] for e in E1], "comb")
    return [m.canonical(a) for a in m.wave_mul(acc, [1] * n, "exit")]


def left_to_right(m, base, e):
    """k_rt_table + k_rt_dual_exp for one exponent: entry, 14 table products, 4 squarings and a window product per window
    below the top one, exit"""
    tab = CM.table16(m, base)
    nw = (e.bit_length() + 3) // 4
    acc = tab[CM.nib(e, nw - 1)] if nw else m.one_m
    for w in range(nw - 2, -1, -1):
        for _ in range(4):
            acc = m.mul(acc, acc, "square")
        acc = m.mul(acc, tab[CM.nib(e, w)], "window")
    return m.canonical(m.mul(acc, 1, "exit"))


def exponent_waves(q, rng):
    edge = [0, 1, 15, 16, 1 << 3071, TOP, q - 1, q - 2, 1 << 2048]
    while len(edge) < 16:
        edge.append(rng.randrange(1 << 3072))
    mixed = [5] + [rng.getrandbits(3072) | (1 << 3071)] + [rng.getrandbits(64) for _ in range(3)]
    top_only = [rng.randrange(1, 16) << (4 * (ROWS - 1))] + [0] * 15
    return [edge, mixed, top_only, [0], [0] * 16]


@pytest.fixture(scope="module")
def comb15():
    m = LazyWide(WH.group15())
    return m, comb_build(m, 4)


def test_lazy_product_is_the_limb_level_product_at_27():
    rng = random.Random(5)
    q = WH.group15()
    m = LazyWide(q)
    for sq in (False, True):
        a = rng.randrange(2 * q)
        b = a if sq else rng.randrange(2 * q)
        want = LM.val(LM.mont_model(LM.limbs(a, L), LM.limbs(b, L), q, LPL, L, {"maxacc": 0}, square=sq))
        assert m.mul(a, b) == want


def test_comb_model_equals_pow_at_768_windows(comb15):
    m, comb = comb15
    q = m.q
    assert m.ops["build"] == 4 * (ROWS - 1) + 14 * ROWS == 3068 + 10752
    assert all(comb[k][d] % q == pow(4, d << (4 * k), q) * m.R % q for k in (0, 1, 511, 512, 767) for d in range(16))
    for E in exponent_waves(q, random.Random(15)):
        assert comb_exp_wave(m, comb, E) == [pow(4, e, q) for e in E]


@pytest.mark.parametrize("mutant", ["row base ^8", "entry d off by one", "phase B from k = 1"])
def test_the_exponent_set_catches_each_mutant_at_768_windows(mutant):
    q = WH.odd_2049()
    m = LazyWide(q)
    comb = comb_build(m, 4, mutant)
    wrong = 0
    for E in exponent_waves(q, random.Random(9)):
        wrong += comb_exp_wave(m, comb, E, mutant=mutant) != [pow(4, e, q) for e in E]
    assert wrong >= 1, mutant


def test_operation_counts_at_3072_bits(comb15):
    m, comb = comb15
    q = m.q
    before = dict(m.ops)
    assert comb_exp_wave(m, comb, [TOP] * 16) == [pow(4, TOP, q)] * 16
    fixed = {k: m.ops[k] - before[k] for k in m.ops}
    assert fixed == {"entry": 0, "build": 0, "table": 0, "square": 0, "window": 0, "comb": 768, "exit": 1}
    assert sum(fixed.values()) == 769
    m2 = LazyWide(q)
    assert left_to_right(m2, 4, TOP) == pow(4, TOP, q)
    assert m2.ops == {"entry": 1, "build": 0, "table": 14, "square": 3068, "window": 767, "comb": 0, "exit": 1}
    assert sum(m2.ops.values()) == 3851
    r1, r2, ops = twin_model(q, L, 3, TOP, TOP)
    assert (r1, r2) == (pow(3, TOP, q),) * 2
    assert ops == {"entry": 1, "square": 3068, "bucket": 1536, "combine": 56, "exit": 2}
    assert sum(ops.values()) == 4663


def test_twin_model_equals_pow_at_3072_bits():
    rng = random.Random(31)
    q = WH.group15()
    for e1, e2 in [(0, TOP), (1 << 2048, 3), (rng.getrandbits(3072), rng.getrandbits(2049))]:
        for base in (0, q - 1, q + 1, TOP, rng.getrandbits(3072)):
            r1, r2, _ = twin_model(q, L, base, e1, e2)
            assert (r1, r2) == (pow(base, e1, q), pow(base, e2, q))
