"""Integer model of the fixed-base comb of a run-time MODP group (mpvss_rs_amd/csrc/modp_rt_kernels.hip): the build
(k_rt_comb_bases / k_rt_comb_rows) and both phases of k_rt_comb_exp, one wave of up to 16 numbers at a time, at each width's
R = 2^(29 L).  Every product is the lazy Montgomery product of bn::mont_mul as an integer -- (a b + m N) / R with operands and
result in [0, 2N), never reduced inside a chain (tests/test_modp_rt_model.py proves the limb-level routine computes exactly
this value) -- and every Montgomery operation a wave issues is counted; the counts are the figures DESIGN section 13 quotes.
No GPU, no library."""
import os
import random
import re

import pytest

import modp_rt_helpers as H
import test_modp_rt_model as LM
from test_modp_rt_twin_model import twin_model

WIDTHS = {5: 20, 9: 36, 18: 72}          # limbs per lane -> L
ROWS = 512
TOP = (1 << 2048) - 1


class Lazy:
    """Montgomery arithmetic of one width with values kept in [0, 2q)"""

    def __init__(self, q, lpl):
        self.q, self.lpl, self.L = q, lpl, WIDTHS[lpl]
        self.rbits = 29 * self.L
        self.R = 1 << self.rbits
        assert self.R > 4 * q
        self.ninv = (-pow(q, -1, self.R)) % self.R
        self.one_m = self.R % q
        self.in_bits = 29 * LM.in_rows(lpl)
        self.kin = pow(2, self.in_bits + self.rbits, q)
        self.ops = {"entry": 0, "build": 0, "table": 0, "square": 0, "window": 0, "comb": 0, "exit": 0}

    def mul(self, a, b, kind=None):
        """one lazy product; kind: count it (a wave's step counts once for its 16 numbers: wave_mul)"""
        assert a < 2 * self.q and b < 2 * self.q
        if kind:
            self.ops[kind] += 1
        t = a * b
        t = (t + ((t * self.ninv) & (self.R - 1)) * self.q) >> self.rbits
        assert t < 2 * self.q
        return t

    def to_mont_in(self, x):
        """the long product that takes any 256-byte value into the width: x kin / 2^(29 IN_ROWS) = x R mod q, below 2q"""
        assert 0 <= x <= TOP
        self.ops["entry"] += 1
        RI = 1 << self.in_bits
        t = x * self.kin
        t = (t + ((t * ((-pow(self.q, -1, RI)) % RI)) & (RI - 1)) * self.q) >> self.in_bits
        assert t < 2 * self.q and t % self.q == x * self.R % self.q
        return t

    def wave_mul(self, A, B, kind):
        self.ops[kind] += 1
        return [self.mul(a, b) for a, b in zip(A, B)]

    def canonical(self, a):
        return a - self.q if a >= self.q else a


def comb_build(m, base, mutant=None):
    """comb[k][d] = base^(d 16^k) R: k_rt_comb_bases walks the row bases (a row base every four squarings, entry 0 of every row),
    k_rt_comb_rows fills d = 2 .. 15"""
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


def table16(m, base):
    """k_rt_table: tab[d] = base^d R"""
    b = m.to_mont_in(base)
    tab = [m.one_m, b]
    for _ in range(2, 16):
        tab.append(m.mul(tab[-1], b, "table"))
    return tab


def nib(e, w):
    return (e >> (4 * w)) & 15


def comb_exp_wave(m, comb, E1, tabs2=None, E2=None, mutant=None):
    """k_rt_comb_exp for one wave: the canonical results of up to 16 numbers.  An operation the wave issues counts once."""
    n = len(E1)
    assert 1 <= n <= 16 and all(0 <= e <= TOP for e in E1)
    acc = [m.one_m] * n
    if tabs2 is not None:                                      # phase A: left to right over B2's table, squarings shared
        nw2 = (max(e.bit_length() for e in E2) + 3) // 4
        if nw2:
            acc = [tabs2[i][nib(E2[i], nw2 - 1)] for i in range(n)]
            for w in range(nw2 - 2, -1, -1):
                for _ in range(4):
                    acc = m.wave_mul(acc, acc, "square")
                acc = m.wave_mul(acc, [tabs2[i][nib(E2[i], w)] for i in range(n)], "window")
    nw1 = (max(e.bit_length() for e in E1) + 3) // 4            # phase B: no squarings
    assert nw1 <= ROWS
    for k in range(1 if mutant == "phase B from k = 1" else 0, nw1):
        if all(nib(e, k) == 0 for e in E1):
            continue                                           # the ballot: digit 0 in the whole wave
        acc = m.wave_mul(acc, [comb[k][nib(e, k)] for e in E1], "comb")
    return [m.canonical(a) for a in m.wave_mul(acc, [1] * n, "exit")]


def moduli():
    sp = H.small_safe_primes()
    return [(5, sp[40]), (5, sp[256]), (9, H.rfc_prime(1024)), (18, H.rfc_prime(1536)), (18, H.rfc_prime(2048))]


def exponent_waves(q, rng):
    """the exponent cases of tests/test_gpu_modp_rt_comb.py, as waves of at most 16"""
    edge = [0, 1, 15, 16, 1 << 2047, TOP, q - 1, q - 2]
    while len(edge) < 16:
        edge.append(rng.randrange(q + 1, 1 << 2048))
    mixed = [5] + [rng.getrandbits(2048) | (1 << 2047)] + [rng.getrandbits(64) for _ in range(3)]
    skip = [sum(rng.randrange(16) << (4 * w) for w in range(0, 512, 3)) for _ in range(16)]     # digit 0 in two windows of three
    top_only = [rng.randrange(1, 16) << (4 * 511)] + [0] * 15
    return [edge, mixed, skip, top_only, [0], [0] * 16]


def bases_for(q, rng):
    return [4, 2, 1, rng.randrange(2, q - 1), q + rng.randrange(1, 1000) if q.bit_length() < 2048 else TOP, q]


def test_lazy_product_is_the_limb_level_product():
    """the integer product used here equals bn::mont_mul's limb model value for value (not only mod q)"""
    rng = random.Random(3)
    for lpl, q in moduli()[1:3]:
        m = Lazy(q, lpl)
        for sq in (False, True):
            a = rng.randrange(2 * q)
            b = a if sq else rng.randrange(2 * q)
            want = LM.val(LM.mont_model(LM.limbs(a, m.L), LM.limbs(b, m.L), q, lpl, m.L, {"maxacc": 0}, square=sq))
            assert m.mul(a, b, "square" if sq else "comb") == want


@pytest.mark.parametrize("lpl,q", moduli(), ids=[f"{q.bit_length()}b" for _, q in moduli()])
def test_model_equals_pow(lpl, q):
    rng = random.Random(q & 0xFFFF)
    for base in bases_for(q, rng):
        m = Lazy(q, lpl)
        comb = comb_build(m, base)
        assert m.ops["build"] == 4 * (ROWS - 1) + 14 * ROWS
        assert all(comb[k][d] % q == pow(base, d << (4 * k), q) * m.R % q for k in (0, 1, 77, 511) for d in range(16))
        for E in exponent_waves(q, rng):
            assert comb_exp_wave(m, comb, E) == [pow(base, e, q) for e in E], (base, E)


@pytest.mark.parametrize("lpl,q", [moduli()[1], moduli()[2], moduli()[4]], ids=["256b", "1024b", "2048b"])
def test_dual_form_equals_pow(lpl, q):
    """a1 = g^r h^c: shared c of 0, 1, 256 bits and full width, per-share c, r = 0, h = 0 mod q"""
    rng = random.Random(lpl)
    m = Lazy(q, lpl)
    comb = comb_build(m, 4)
    for n in (1, 16):
        Hs = [rng.randrange(1 << 2048) for _ in range(n)]
        Hs[0] = q
        tabs = [table16(m, h) for h in Hs]
        R_ = [rng.randrange(1 << 2048) for _ in range(n)]
        R_[-1] = 0
        for C in ([0] * n, [1] * n, [rng.getrandbits(256)] * n, [TOP] * n, [rng.randrange(q) for _ in range(n)]):
            got = comb_exp_wave(m, comb, R_, tabs, C)
            assert got == [pow(4, r, q) * pow(h, c, q) % q for r, h, c in zip(R_, Hs, C)], (n, C[0])


@pytest.mark.parametrize("mutant", ["row base ^8", "entry d off by one", "phase B from k = 1"])
def test_the_exponent_set_catches_each_mutant(mutant):
    lpl, q = moduli()[1]
    rng = random.Random(9)
    m = Lazy(q, lpl)
    comb = comb_build(m, 4, mutant)
    wrong = 0
    for E in exponent_waves(q, rng):
        wrong += comb_exp_wave(m, comb, E, mutant=mutant) != [pow(4, e, q) for e in E]
    assert wrong >= 1, mutant


def test_operation_counts_are_the_documented_figures():
    q = H.rfc_prime(2048)
    m = Lazy(q, 18)
    comb = comb_build(m, 4)
    build = dict(m.ops)
    assert build["entry"] == 1 and build["build"] == 2044 + 7168
    # g^e with a full-width exponent: 512 comb products + 1 exit, no squaring
    comb_exp_wave(m, comb, [TOP] * 16)
    fixed = {k: m.ops[k] - build[k] for k in m.ops}
    assert fixed == {"entry": 0, "build": 0, "table": 0, "square": 0, "window": 0, "comb": 512, "exit": 1}
    g_e = sum(fixed.values())
    assert g_e == 513
    # what it replaces: the left-to-right chain over the base's 16-entry table, 2 044 squarings + 511 window products
    today = 4 * 511 + 511
    assert today == 2555
    twin = sum(twin_model(q, 72, 3, TOP, TOP)[2].values())
    assert twin == 3127
    dealer, extract = 2 * g_e + twin, twin + g_e                       # (X, a1, twin) and (twin, a1)
    assert (dealer, extract) == (4153, 3640)
    assert (2 * today + twin, twin + today) == (8237, 5682)
    # the verifier's a1 = g^r X^c with a 256-bit c: X's table (1 entry + 14), 63 windows of c with 4 squarings each, then
    # the comb over r at full width and the exit
    m2 = Lazy(q, 18)
    tab = table16(m2, 12345)
    comb_exp_wave(m2, comb, [TOP], [tab], [(1 << 256) - 1])
    assert m2.ops == {"entry": 1, "build": 0, "table": 14, "square": 252, "window": 63, "comb": 512, "exit": 1}
    a1 = sum(m2.ops.values())
    assert a1 == 843
    # today the shared squarings run as long as r: 2 044 squarings + 511 + 512 window products + table, entry and exit
    assert 2044 + 511 + 512 + 14 + 1 + 1 == 3083
    design = open(os.path.join(os.path.dirname(H.HERE), "DESIGN.md")).read()
    sec13 = design[design.index("## 13"):]
    for figure in (r"\b513\b", r"\b4 ?153\b", r"\b3 ?640\b", r"\b843\b", r"\b2 ?555\b"):
        assert re.search(figure, sec13), f"DESIGN section 13 must quote the model's count {figure}"


def test_cost_follows_the_operands():
    q = H.small_safe_primes()[256]
    m = Lazy(q, 5)
    comb = comb_build(m, 2)
    before = dict(m.ops)
    comb_exp_wave(m, comb, [0] * 16)
    assert m.ops["comb"] == before["comb"] and m.ops["exit"] == before["exit"] + 1
    comb_exp_wave(m, comb, [(1 << 64) - 1, 5])
    assert m.ops["comb"] == before["comb"] + 16
    # the skip: one non-zero digit in the wave, in window 511
    comb_exp_wave(m, comb, [7 << 2044] + [0] * 15)
    assert m.ops["comb"] == before["comb"] + 17
