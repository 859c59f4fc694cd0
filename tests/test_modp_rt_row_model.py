"""Integer model of the run-time row-layout Montgomery product (mpvss_rs_amd/csrc/bn_row_rt.h: 16 lanes per number) at the three
widths it is instantiated at -- (L, row LPL) = (72, 5), (108, 7), (144, 9), the handles of 18 / 27 / 36 quad limbs per lane -- and of
the step programs of k_rt_dual_exp_row / k_rt_comb_exp_row (modp_rt_row_kernels.hip) with their operation counts.  No GPU."""
import math
import random

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import modp_rt_4096_helpers as XH
from test_modp_rt_model import LIMB_BOUND, M, W, limbs, mont_model, val
from test_modp_rt_4096_model import mont_model36, new_stats as new_stats36

LANES = 16
WIDTHS = ((72, 5), (108, 7), (144, 9))           # (L, row LPL); quad LPL = L / 4
EB = {72: 256, 108: 384, 144: 512}


def row_rt_model(a, b, N, L, lpl, stats, square=False, bound_only=False):
    """bnrowrt::mont_mul<lpl, L, square> as integers, same step order: 16 lpl column slots (slots >= L hold zeros on input), L rows
    (L // lpl rolled groups of lpl rows, then L % lpl tail rows: the accumulators end rotated by L % lpl), n0inv a run-time value;
    every lane carries its lowest column every row and hands its low 29 bits to the lane below; two final carry passes.
    stats: maxacc, the largest accumulator; units, the most product units (a doubled limb counts two) a column collected
    between two carries; cout, the largest carry-out of a lane in the final pass."""
    cols = LANES * lpl
    assert L <= cols
    a = list(a) + [0] * (cols - L)
    nl = limbs(N, L) + [0] * (cols - L)
    n0inv = (-pow(N, -1, 1 << W)) % (1 << W)
    T, U = [0] * cols, [0] * cols
    rows = 0
    for i in range(L):
        bi = b[i]
        rr = i % lpl
        for j in range(cols):
            k = j % lpl
            if not square:
                T[j] += a[j] * bi
                U[j] += 1
            elif k >= rr:
                T[j] += a[j] * (2 * bi if k > rr else bi)
                U[j] += 2 if k > rr else 1
        m = ((T[0] & 0xFFFFFFFF) * n0inv) & M              # (u32)T[RR] * n0inv, masked
        for j in range(cols):
            T[j] += m * nl[j]
            U[j] += 1
        assert T[0] & M == 0
        stats["maxacc"] = max(stats["maxacc"], max(T))
        stats["units"] = max(stats["units"], max(U))
        for q in range(LANES):
            j = q * lpl
            T[j + 1] += T[j] >> W
            T[j] &= M
        stats["maxacc"] = max(stats["maxacc"], max(T))
        T = T[1:] + [0]
        U = U[1:] + [0]
        for q in range(LANES):
            U[q * lpl + lpl - 1] = 0                       # a lane's fresh top column: 29 bits from the lane above, or zero
        rows += 1
    assert rows % lpl == L % lpl                           # the tail rotation the final pass undoes
    if bound_only:
        return None
    out, couts = [0] * cols, [0] * LANES
    for q in range(LANES):
        c = 0
        for k in range(lpl):
            v = T[q * lpl + k] + c
            out[q * lpl + k] = v & M
            c = v >> W
        couts[q] = c
    stats["cout"] = max(stats["cout"], max(couts))
    assert couts[LANES - 1] == 0
    for q in range(1, LANES):
        v = out[q * lpl] + couts[q - 1]
        out[q * lpl] = v & M
        out[q * lpl + 1] += v >> W
    assert all(x == 0 for x in out[L:])
    return out[:L]


def new_stats():
    return {"maxacc": 0, "units": 0, "cout": 0}


def quad_model(a, b, N, L, square):
    """the quad layout's product of the same operands (tests/test_modp_rt_model.py's pipeline; its 36-limb form at L = 144)"""
    if L == 144:
        return mont_model36(a, b, N, L, new_stats36(), square=square)
    return mont_model(a, b, N, L // 4, L, {"maxacc": 0}, square=square)


def moduli(L):
    rfc = {72: int(O.MODP_Q_HEX, 16), 108: WH.group15(), 144: XH.group16()}[L]
    # (both end in ones, n0inv = 1: a random odd modulus of the width's capacity exercises the run-time multiply)
    return [(1 << (W * L - 2)) - 1, rfc, H.random_odd_modulus(W * L - 2, random.Random(1000 + L))]


def worst_vector(L, N):
    """every limb at the almost-normalised bound, the top ones lowered until the value is below 2N"""
    v = [LIMB_BOUND] * L
    j = L - 1
    while val(v) >= 2 * N:
        if v[j] == 0:
            j -= 1
        v[j] //= 2
    return v


def test_the_widths():
    for L, lpl in WIDTHS:
        assert L <= LANES * lpl < L + lpl + (8 if lpl == 5 else 0)
        assert L % lpl == {5: 2, 7: 3, 9: 0}[lpl]
    assert int(O.MODP_Q_HEX, 16).bit_length() == 2048 and WH.group15().bit_length() == 3072 and XH.group16().bit_length() == 4096


# log2 of the largest accumulator, (product, squaring), that DESIGN section 13 and bn_row_rt.h quote
FIGURES = {
    "equal": {5: (60.44, 60.44), 7: (60.93, 60.93), 9: (61.30, 61.30)},
    "mixed": {5: (61.06, 61.06), 7: (61.51, 61.51), 9: (61.96, 61.98)},
}


def bound_vectors(L):
    """operands far above 2N as integers, for the accumulator bound only.  equal: every limb at 2^29 - 1 + 2^9 -- every product
    term at its maximum, but m of every row comes out small; mixed: four limbs in five at the bound, the others random (seeded),
    which gives rows with m near 2^29 and the larger columns"""
    rng = random.Random(L)
    return {"equal": [LIMB_BOUND] * L, "mixed": [LIMB_BOUND if rng.random() < 0.8 else rng.randrange(LIMB_BOUND) for _ in range(L)]}


@pytest.mark.parametrize("L,lpl", WIDTHS)
def test_worst_case_limbs_stay_below_2_63(L, lpl):
    """Limbs at 2^29 - 1 + 2^9 (bound check only).  Between two carries a column collects at most 2 lpl product units in the
    product AND in the squaring (its rows visit k >= rr only, the doubled limbs count two: the model counts them), each below
    2^58.01: below 2^61.33 / 2^61.82 / 2^62.18 at lpl 5 / 7 / 9 with the carry that came in, so no second carry at any width."""
    N = (1 << (W * L - 2)) - 1
    analytic = math.log2(2 * lpl * LIMB_BOUND * LIMB_BOUND + (1 << 40))
    assert analytic < {5: 61.34, 7: 61.83, 9: 62.19}[lpl]
    for name, vec in bound_vectors(L).items():
        figures = []
        for sq in (False, True):
            stats = new_stats()
            row_rt_model(vec, vec, N, L, lpl, stats, square=sq, bound_only=True)
            assert stats["maxacc"] < (1 << 63)
            assert stats["units"] == 2 * lpl
            figures.append(math.log2(stats["maxacc"]))
        print(f"L={L} lpl={lpl} {name}: largest accumulator 2^{figures[0]:.2f} (product) 2^{figures[1]:.2f} (squaring)")
        assert max(figures) < analytic
        assert all(abs(f - w) < 0.01 for f, w in zip(figures, FIGURES[name][lpl])), (name, figures)


@pytest.mark.parametrize("L,lpl", WIDTHS)
def test_product_and_squaring_match_montgomery_and_the_quad_model(L, lpl):
    rng = random.Random(L)
    R = 1 << (W * L)
    n0invs = set()
    stats = new_stats()
    for N in moduli(L):
        assert 4 * N < R
        n0invs.add((-pow(N, -1, 1 << W)) % (1 << W))
        rinv = pow(R, -1, N)
        worst = worst_vector(L, N)
        named = [limbs(2 * N - 1, L), worst, limbs(0, L), limbs(1, L), limbs(N, L)]
        cases = [(a, b) for a in named for b in named]
        cases += [(limbs(rng.randrange(2 * N), L), limbs(rng.randrange(2 * N), L)) for _ in range(6)]
        for a, b in cases:
            for sq in (False, True):
                bb = a if sq else b
                r = row_rt_model(a, bb, N, L, lpl, stats, square=sq)
                v = val(r)
                assert v < 2 * N and v % N == val(a) * val(bb) * rinv % N
                assert max(r) <= LIMB_BOUND
                assert v == val(quad_model(a, bb, N, L, sq))
    assert stats["maxacc"] < (1 << 63)
    assert stats["cout"] < (1 << 37)
    assert len(n0invs - {1}) >= 1, "the run-time n0inv must be exercised with a value other than 1"


# ---- the step programs of the two kernels, on Python integers, with their operation counts -----------------------------------
def nib(e, w):
    return (e >> (4 * w)) & 15


def tables(q, bases):
    """k_rt_table: the 16 powers of every base"""
    return [[pow(b, d, q) for d in range(16)] for b in bases]


def comb_rows(q, g, rows):
    """k_rt_comb_*: comb[k][d] = g^(d 16^k)"""
    out = []
    for _ in range(rows):
        row = [1, g]
        for _ in range(14):
            row.append(row[-1] * g % q)
        out.append(row)
        g = row[15] * g % q
    return out


def dual_exp_row_wave(q, B1, E1, B2=None, E2=None):
    """k_rt_dual_exp_row for the numbers of one wave: (results, squarings, products) on one number's chain"""
    nb = max(e.bit_length() for e in E1 + (E2 or []))
    nw = (nb + 3) // 4
    if nw == 0:
        return [1] * len(B1), 0, 0
    w = nw - 1
    T1, T2 = tables(q, B1), tables(q, B2 or [])
    acc = [t[nib(e, w)] for t, e in zip(T1, E1)]
    sq = mul = 0
    s = 5 if B2 else 6
    while True:
        if s == 6:
            if w == 0:
                break
            w -= 1
            s = 0
        if s < 4:
            acc = [x * x % q for x in acc]
            sq += 1
        elif s == 4:
            acc = [x * t[nib(e, w)] % q for x, t, e in zip(acc, T1, E1)]
            mul += 1
        else:
            acc = [x * t[nib(e, w)] % q for x, t, e in zip(acc, T2, E2)]
            mul += 1
        s += 1
        if s == 5 and not B2:
            s = 6
    return acc, sq, mul


def comb_exp_row_wave(q, g, E1, B2=None, E2=None):
    """k_rt_comb_exp_row for the numbers of one wave: (results, squarings, products)"""
    nw1 = (max(e.bit_length() for e in E1) + 3) // 4
    nw2 = (max(e.bit_length() for e in E2) + 3) // 4 if B2 else 0
    sq = mul = 0
    w, k = nw2 - 1, 0
    T2, comb = tables(q, B2 or []), comb_rows(q, g, nw1)
    if nw2 == 0:
        acc, s = [1] * len(E1), 6
    else:
        acc, s = [t[nib(e, w)] for t, e in zip(T2, E2)], 5
    while True:
        if s == 5:
            if w == 0:
                s = 6
            else:
                w -= 1
                s = 0
        if s == 6:
            while k < nw1 and all(nib(e, k) == 0 for e in E1):
                k += 1
            if k == nw1:
                break
        if s < 4:
            acc = [x * x % q for x in acc]
            sq += 1
        elif s == 4:
            acc = [x * t[nib(e, w)] % q for x, t, e in zip(acc, T2, E2)]
            mul += 1
        else:
            acc = [x * comb[k][nib(e, k)] % q for x, e in zip(acc, E1)]
            k += 1
            mul += 1
        if s < 5:
            s += 1
    return acc, sq, mul


@pytest.mark.parametrize("L,lpl", WIDTHS)
def test_step_programs_equal_pow_and_their_operation_counts(L, lpl):
    """One number's chain at full-width exponents (the row kernel's own operations; modp_rt_launch_from_mont adds one product):
    dual_exp 4 (2 EB - 1) squarings + (2 EB - 1) products, + 2 EB with a second table; comb_exp 2 EB products and no squaring,
    with a 256-bit e2 over tab2 252 squarings + 63 products more."""
    q = moduli(L)[1]
    eb = EB[L]
    rng = random.Random(lpl)
    full = (1 << (8 * eb)) - 1
    B1 = [rng.randrange(2, q) for _ in range(4)]
    B2 = [rng.randrange(2, q) for _ in range(4)]
    E1 = [full, rng.getrandbits(8 * eb), 5, 0]
    E2 = [rng.getrandbits(256) | (1 << 255), 0, 1, rng.getrandbits(200)]
    nw = 2 * eb
    r, sq, mul = dual_exp_row_wave(q, B1, E1)
    assert r == [pow(b, e, q) for b, e in zip(B1, E1)] and (sq, mul) == (4 * (nw - 1), nw - 1)
    r, sq, mul = dual_exp_row_wave(q, B1, E1, B2, E2)
    assert r == [pow(b, e, q) * pow(c, f, q) % q for b, e, c, f in zip(B1, E1, B2, E2)] and (sq, mul) == (4 * (nw - 1), 2 * nw - 1)
    g = B1[0]
    r, sq, mul = comb_exp_row_wave(q, g, E1)
    assert r == [pow(g, e, q) for e in E1] and (sq, mul) == (0, nw)
    r, sq, mul = comb_exp_row_wave(q, g, E1, B2, E2)
    assert r == [pow(g, e, q) * pow(c, f, q) % q for e, c, f in zip(E1, B2, E2)] and (sq, mul) == (4 * 63, 63 + nw)
    # nothing to do: every exponent of the wave 0 (the result is 1, no product); a sparse e1 skips the rows that are 0 everywhere
    assert dual_exp_row_wave(q, B1, [0] * 4) == ([1] * 4, 0, 0)
    assert comb_exp_row_wave(q, g, [0] * 4) == ([1] * 4, 0, 0)
    r, sq, mul = comb_exp_row_wave(q, g, [1 << 40, 1 << 400, 0, 3])
    assert r == [pow(g, e, q) for e in (1 << 40, 1 << 400, 0, 3)] and (sq, mul) == (0, 3)
    counts = {72: (2044, 511, 2044, 1023, 512), 108: (3068, 767, 3068, 1535, 768), 144: (4092, 1023, 4092, 2047, 1024)}[L]
    assert counts == (4 * (nw - 1), nw - 1, 4 * (nw - 1), 2 * nw - 1, nw)
