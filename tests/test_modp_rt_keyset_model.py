"""Integer model of the key sets of a run-time MODP group (mpvss_rs_amd/csrc/modp_rt_kernels.inc): the build
(k_rt_keyset_bases / k_rt_keyset_rows) and the window schedule of k_rt_keyset_exp, one wave of up to 16 numbers at a time, at
each width's R = 2^(29 L), L = 20 / 36 / 72 / 108.  Every product is the lazy Montgomery product of bn::mont_mul as an integer --
operands and result in [0, 2q), never reduced inside a chain (test_modp_rt_comb_model.Lazy asserts the bound at every product) --
and every Montgomery operation a wave issues is counted; the counts are the figures DESIGN section 13 quotes.  No GPU, no
library."""
import os
import random
import re

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import test_modp_rt_comb_model as CM
import test_modp_rt_wide_model as WM
from test_modp_rt_twin_model import twin_model


def lazy(q, lpl):
    m = WM.LazyWide(q) if lpl == 27 else CM.Lazy(q, lpl)
    m.ops["row"] = 0
    m.EB = 384 if lpl == 27 else 256
    m.J = m.EB // 32
    return m


def top(m):
    return (1 << (8 * m.EB)) - 1


def keyset_build(m, key, mutant=None):
    """ks[j][d] = key^(d 2^(256 j)) R: k_rt_keyset_bases squares 256 (J - 1) times and keeps entry 1 of a row every 256
    squarings and entry 0 of every row; k_rt_keyset_rows fills d = 2 .. 15"""
    ks = [[m.one_m] + [0] * 15 for _ in range(m.J)]
    acc = m.to_mont_in(key)
    for j in range(m.J):
        ks[j][1] = acc
        if j + 1 < m.J:
            for _ in range(255 if mutant == "row base 255 squarings" else 256):
                acc = m.mul(acc, acc, "build")
    for j in range(m.J):
        acc = ks[j][1]
        for d in range(2, 16):
            acc = m.mul(acc, ks[j][1], "build")
            ks[j][d] = acc
    return ks


def nib(e, w):
    return (e >> (4 * w)) & 15


def keyset_exp_wave(m, KS, E1, tabs2=None, E2=None, mutant=None):
    """k_rt_keyset_exp for one wave (one exponent set): the canonical results of up to 16 numbers; KS[i] the rows of number i.
    An operation the wave issues counts once."""
    n = len(E1)
    assert 1 <= n <= 16 and all(0 <= e <= top(m) for e in E1)
    nb1 = max(e.bit_length() for e in E1)
    jl = (nb1 + 255) // 256
    nw1 = (min(nb1, 256) + 3) // 4
    nw2 = (max(e.bit_length() for e in E2) + 3) // 4 if tabs2 is not None else 0
    acc, one = [m.one_m] * n, True
    for w in range(max(nw1, nw2) - 1, -1, -1):
        if not one:
            for _ in range(4):
                acc = m.wave_mul(acc, acc, "square")
        if w < (63 if mutant == "rows join at 63" else 64):
            for j in range(jl):
                digits = [nib(e, 64 * j + w) for e in E1]
                if all(d == 0 for d in digits):
                    continue                                   # the ballot: digit 0 in the whole wave
                acc = m.wave_mul(acc, [KS[i][j][d] for i, d in enumerate(digits)], "row")
                one = False
        if w < nw2:
            acc = m.wave_mul(acc, [tabs2[i][nib(E2[i], w)] for i in range(n)], "window")
            one = False
    return [m.canonical(a) for a in m.wave_mul(acc, [1] * n, "exit")]


def moduli():
    sp = H.small_safe_primes()
    return [(5, sp[40]), (5, sp[256]), (9, H.rfc_prime(1024)), (18, H.rfc_prime(1536)), (18, H.rfc_prime(2048)), (27, WH.group15())]


def keys_for(m, rng):
    q, T = m.q, top(m)
    keys = [1, q - 1, q, q + 12345 if q + 12345 <= T else T, T, 2 * q - 1 if 2 * q - 1 <= T else T - 1, rng.randrange(2, q - 1), 0]
    return keys[:5] if m.lpl == 27 else keys                           # the build is 2 985 products a key at that width


def exponent_waves(m, rng):
    """the exponent cases of tests/test_gpu_modp_rt_keyset.py, as waves of at most 16"""
    q, T, J, bits = m.q, top(m), m.J, 8 * m.EB
    edge = [0, 1, 15, 16, 1 << 255, (1 << 256) - 1, 1 << 256, (1 << 256) + 1, 1 << (bits - 1), T, q - 1, q - 2]
    rows = [1 << (256 * j) for j in range(J)]
    tops = [9 << (4 * (64 * j + 63)) for j in range(J)]
    # digits zero in whole rows (every odd row) and in every third window
    sparse = [sum(rng.randrange(1, 16) << (4 * (64 * j + w)) for j in range(0, J, 2) for w in range(64) if w % 3) for _ in range(16)]
    one_live = [0] * 7 + [rng.getrandbits(bits)] + [0] * 8
    mixed = [5, rng.getrandbits(bits) | (1 << (bits - 1)), rng.getrandbits(64), rng.getrandbits(300), rng.getrandbits(255)]
    return [edge, rows, tops, sparse, one_live, mixed, [0], [0] * 16, [rng.getrandbits(100) for _ in range(3)]]


@pytest.mark.parametrize("lpl,q", moduli(), ids=[f"{q.bit_length()}b" for _, q in moduli()])
def test_build_and_schedule_equal_pow(lpl, q):
    """every key kind against every exponent wave; CM.Lazy.mul asserts [0, 2q) at every product on the way"""
    rng = random.Random(q & 0xFFFF)
    m = lazy(q, lpl)
    keys = keys_for(m, rng)
    before = dict(m.ops)
    KS = [keyset_build(m, k) for k in keys]
    assert m.ops["entry"] - before["entry"] == len(keys)
    assert m.ops["build"] == len(keys) * (256 * (m.J - 1) + 14 * m.J)
    for key, ks in zip(keys, KS):
        for j in (0, 1, m.J - 1):
            for d in (0, 1, 2, 15):
                assert ks[j][d] < 2 * q and ks[j][d] % q == pow(key, d << (256 * j), q) * m.R % q
    assert all(v % q == 0 for v in KS[2][3][1:]) and KS[2][0][0] == m.one_m    # a key that is 0 mod q: rows of zeros beside entry 0
    for E in exponent_waves(m, rng):
        for k0 in ((0,) if lpl == 27 else (0, 3)):                      # different keys side by side in one wave
            ks_of = [KS[(k0 + i) % len(KS)] for i in range(len(E))]
            want = [pow(keys[(k0 + i) % len(KS)], e, q) for i, e in enumerate(E)]
            assert keyset_exp_wave(m, ks_of, E) == want, (k0, E)


@pytest.mark.parametrize("lpl,q", [moduli()[1], moduli()[2], moduli()[4], moduli()[5]], ids=["256b", "1024b", "2048b", "3072b"])
def test_dual_form_equals_pow(lpl, q):
    """a2 = y^r Y^c: shared c of 0, 1, 2^256 - 1, 2^256 and all ones (longer than 256 bits: its windows above 64 run before the
    rows join), per-share c, r = 0 and all ones, Y = 0 mod q"""
    rng = random.Random(lpl)
    m = lazy(q, lpl)
    T = top(m)
    for n in ((1, 2) if lpl == 27 else (1, 4)):                        # a 3072-bit pow costs Python tens of milliseconds
        ys = [rng.randrange(T + 1) for _ in range(n)]
        Ys = [rng.randrange(T + 1) for _ in range(n)]
        Ys[0] = q
        KS = [keyset_build(m, y) for y in ys]
        tabs = [CM.table16(m, h) for h in Ys]
        R_ = [rng.randrange(T + 1) for _ in range(n)]
        R_[-1] = 0
        R_[0] = T
        for C in ([0] * n, [1] * n, [(1 << 256) - 1] * n, [1 << 256] * n, [T] * n, [rng.randrange(q) for _ in range(n)]):
            got = keyset_exp_wave(m, KS, R_, tabs, C)
            assert got == [pow(y, r, q) * pow(h, c, q) % q for y, r, h, c in zip(ys, R_, Ys, C)], (n, C[0])
        # a short e1 under a long e2, and the other way round
        assert keyset_exp_wave(m, KS, [3] * n, tabs, [T] * n) == [pow(y, 3, q) * pow(h, T, q) % q for y, h in zip(ys, Ys)]
        assert keyset_exp_wave(m, KS, [T] * n, tabs, [3] * n) == [pow(y, T, q) * pow(h, 3, q) % q for y, h in zip(ys, Ys)]


@pytest.mark.parametrize("mutant", ["row base 255 squarings", "rows join at 63"])
def test_the_exponent_set_catches_each_mutant(mutant):
    lpl, q = moduli()[1]
    rng = random.Random(9)
    m = lazy(q, lpl)
    ks = keyset_build(m, 3, mutant)
    wrong = 0
    for E in exponent_waves(m, rng):
        wrong += keyset_exp_wave(m, [ks] * len(E), E, mutant=mutant) != [pow(3, e, q) for e in E]
    assert wrong >= 1, mutant


def test_operation_counts_are_the_documented_figures():
    q = H.rfc_prime(2048)
    m = lazy(q, 18)
    T = top(m)
    ks = keyset_build(m, 12345)
    assert (m.ops["entry"], m.ops["build"]) == (1, 256 * 7 + 14 * 8)
    build = m.ops["entry"] + m.ops["build"]
    assert build == 1905
    # a2 = y^r Y^c, r of full width and c of 256 bits: Y's table, 63 x 4 squarings, 64 x (8 rows + 1 window of c), the exit
    m2 = lazy(q, 18)
    tab = CM.table16(m2, 54321)
    keyset_exp_wave(m2, [ks], [T], [tab], [(1 << 256) - 1])
    assert m2.ops == {"entry": 1, "build": 0, "table": 14, "square": 252, "window": 64, "comb": 0, "row": 512, "exit": 1}
    a2 = sum(m2.ops.values())
    assert a2 == 844
    a2_today = 2044 + 511 + 512 + 14 + 1 + 1
    assert a2_today == 3083
    # the dealer's two powers of a key: two exponent sets of full width, 252 squarings + 512 row products + exit each
    m3 = lazy(q, 18)
    keyset_exp_wave(m3, [ks], [T])
    one_set = sum(m3.ops.values())
    assert m3.ops["square"] == 252 and m3.ops["row"] == 512 and one_set == 765
    twin, twin_today = 2 * one_set, sum(twin_model(q, 72, 3, T, T)[2].values())
    assert (twin, twin_today) == (1530, 3127)
    # whole shares: the verifier at t = 256 with forward differences (X 255, a1 843) and under Horner's rule, the dealer (two g^e of 513)
    assert (255 + 843 + a2_today, 255 + 843 + a2) == (4181, 1942)
    assert (9526 - a2_today + a2,) == (7287,)
    assert (2 * 513 + twin_today, 2 * 513 + twin) == (4153, 2556)
    # 3072 bits: 12 rows
    mw = lazy(WH.group15(), 27)
    ksw = keyset_build(mw, 12345)
    assert mw.ops["entry"] + mw.ops["build"] == 1 + 256 * 11 + 14 * 12 == 2985
    keyset_exp_wave(mw, [ksw], [top(mw)])
    assert mw.ops["square"] == 252 and mw.ops["row"] == 768
    design = open(os.path.join(os.path.dirname(H.HERE), "DESIGN.md")).read()
    sec13 = design[design.index("## 13"):]
    for figure in (r"\b1 ?905\b", r"\b844\b", r"\b1 ?530\b", r"\b1 ?942\b", r"\b2 ?556\b", r"\b7 ?287\b", r"\b2 ?985\b"):
        assert re.search(figure, sec13), f"DESIGN section 13 must quote the model's count {figure}"


def test_bytes_per_key():
    assert [(256 // 32) * 16 * 4 * lpl * 4 for lpl in (5, 9, 18)] + [(384 // 32) * 16 * 4 * 27 * 4] == [10240, 18432, 36864, 82944]


def test_cost_follows_the_operands():
    q = H.small_safe_primes()[256]
    m = lazy(q, 5)
    ks = keyset_build(m, 2)
    before = dict(m.ops)
    keyset_exp_wave(m, [ks] * 16, [0] * 16)                              # nothing but the exit
    assert {k: m.ops[k] - before[k] for k in m.ops} == {"entry": 0, "build": 0, "table": 0, "square": 0, "window": 0, "comb": 0,
                                                         "row": 0, "exit": 1}
    before = dict(m.ops)
    keyset_exp_wave(m, [ks] * 2, [(1 << 64) - 1, 5])                     # 16 windows of row 0, squarings after the first product
    assert (m.ops["row"] - before["row"], m.ops["square"] - before["square"]) == (16, 60)
    before = dict(m.ops)
    keyset_exp_wave(m, [ks] * 16, [1 << 2044] + [0] * 15)               # one digit, in row 7: no squaring before it, 4 x 63 after
    assert (m.ops["row"] - before["row"], m.ops["square"] - before["square"]) == (1, 252)
    before = dict(m.ops)
    keyset_exp_wave(m, [ks] * 16, [1 << 1792] + [0] * 15)               # the lowest digit of row 7: one product, no squaring
    assert (m.ops["row"] - before["row"], m.ops["square"] - before["square"]) == (1, 0)
