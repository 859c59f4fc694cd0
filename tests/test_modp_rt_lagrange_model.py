"""Integer model of the Lagrange exponents of a run-time MODP group on the device (k_rt_lagrange_terms, the Fermat power through
k_rt_table and k_rt_dual_exp, k_rt_lagrange_finish in mpvss_rs_amd/csrc/modp_rt_kernels.inc), in the manner of
tests/test_modp_rt_scalar_model.py: residues mod q' = (q-1)/2 in the lazy [0, 2 q') Montgomery product at the handle's width.

The model is exact integers: a product of `rows` rows is (a b + m N) / 2^(29 rows) with m = -a b / N mod 2^(29 rows), what the
CIOS loop of bn::mont_mul computes, below N + a b / 2^(29 rows).  It asserts the bound of the quarter product (rows = limbs per
lane, the second operand a factor of three limbs) at every width and for q' = 11, that the stray power of two cancels, the check
den den^-1 = 1 with what it catches, the store rule with a magnitude 0 under a negative sign, and the product counts per
coefficient.  No library, no GPU."""
import math

import pytest

import modp_rt_4096_helpers as H4
import modp_rt_helpers as H
import modp_rt_lagrange_cases as LC
import modp_rt_wide_helpers as WH

W = 29
LPLS = (5, 9, 18, 27, 36)
EB = {5: 256, 9: 256, 18: 256, 27: 384, 36: 512}


class Ring:
    """the constants of q' at a width of lpl limbs per lane and the three steps"""

    def __init__(self, q, lpl):
        assert q % 4 == 3 and q >= 7
        self.q, self.N, self.lpl = q, (q - 1) // 2, lpl
        self.L, self.EB = 4 * lpl, EB[lpl]
        self.IN_ROWS = lpl * (((8 * self.EB + 28) // 29 + lpl - 1) // lpl)
        self.R = 1 << (W * self.L)
        assert self.R > 8 * self.N
        self.kin = pow(2, W * (self.IN_ROWS + self.L), self.N)
        self.one_m = self.R % self.N
        self.quarter = self.full = self.entry = 0
        self._ninv = {}

    def mont(self, a, b, rows):
        Rr = 1 << (W * rows)
        if rows not in self._ninv:
            self._ninv[rows] = pow(self.N, -1, Rr)
        m = (-a * b * self._ninv[rows]) % Rr
        t, rem = divmod(a * b + m * self.N, Rr)
        assert rem == 0 and t < self.N + a * b // Rr + 1
        return t

    def step(self, acc, factor):
        """the quarter product: acc < 2 q' (almost normalised limbs: the value is what counts), factor three limbs"""
        assert acc < 2 * self.N and 0 <= factor < 1 << (3 * W)
        self.quarter += 1
        r = self.mont(acc, factor, self.lpl)
        assert r < 2 * self.N
        return r

    def product(self, a, b):
        assert a < 2 * self.N and b < 2 * self.N
        self.full += 1
        r = self.mont(a, b, self.L)
        assert r < 2 * self.N
        return r

    def to_mont_in(self, x):
        assert 0 <= x < 1 << (8 * self.EB)
        self.entry += 1
        r = self.mont(self.kin, x, self.IN_ROWS)
        assert r < 2 * self.N and r % self.N == x * self.R % self.N
        return r

    def terms(self, xs, i):
        """k_rt_lagrange_terms for quad i: (num, den), both below 2 q'"""
        num = den = self.one_m
        for j in range(len(xs) - 1):
            jj = j + (1 if j >= i else 0)                  # the quad's own index skipped, m - 1 steps for every quad
            num = self.step(num, xs[jj])
            den = self.step(den, abs(xs[jj] - xs[i]))
        return num, den

    def fermat(self, den, windows=True):
        """k_rt_table and k_rt_dual_exp with the exponent q' - 2 over the denominator's canonical bytes: 4-bit windows from the
        highest one, left to right; the result canonical.  Counts the entry, the table's 14 products, squarings, window products
        and the exit as full products.  windows=False: Python's pow in place of the window loop (the wide moduli, where the loop
        of big-integer products takes seconds per coefficient; test_product_counts_per_coefficient walks it once per width)."""
        d = den % self.N
        if not windows:
            return pow(d, self.N - 2, self.N)
        b = self.to_mont_in(d)
        tab = [self.one_m % self.N, b]
        for _ in range(14):
            tab.append(self.product(tab[-1], b))
        e = self.N - 2
        nw = (e.bit_length() + 3) // 4
        if nw == 0:
            acc = self.one_m
        else:
            acc = tab[(e >> (4 * (nw - 1))) & 15]
            for w in range(nw - 2, -1, -1):
                for _ in range(4):
                    acc = self.product(acc, acc)
                acc = self.product(acc, tab[(e >> (4 * w)) & 15])
        acc = self.product(acc, 1)
        r = acc % self.N
        assert r == pow(d, self.N - 2, self.N)
        return r

    def finish(self, num, den, dinv, negative):
        """k_rt_lagrange_finish: (flag, exponent)"""
        t = self.to_mont_in(dinv)
        check = self.product(den, t) % self.N
        mag = self.product(num, t) % self.N
        return check == 1 % self.N, self.store(mag, negative)

    def store(self, mag, negative):
        assert 0 <= mag < self.N
        return mag if (not negative or mag == 0) else 2 * self.N - mag

    def exponents(self, xs):
        """(flags, exponents) of a list"""
        neg = LC.signs(xs)
        out = []
        for i in range(len(xs)):
            num, den = self.terms(xs, i)
            out.append(self.finish(num, den, self.fermat(den, windows=self.q.bit_length() <= 256), neg[i]))
        return [f for f, _ in out], [e for _, e in out]


def _moduli():
    sp = H.small_safe_primes()
    return [(23, 5), (sp[40], 5), (H.rfc_prime(1024), 9), (H.rfc_prime(2048), 18), (WH.group15(), 27), (H4.group16(), 36)]


MODULI = _moduli()
IDS = [f"{q.bit_length()}b" for q, _ in MODULI]


def test_the_widths_are_the_five_instantiated_ones():
    assert tuple(lpl for _, lpl in MODULI[1:]) == LPLS
    assert [LC.HANDLES[k][2] for k in LC.KEYS] == list(LPLS)


# every modulus at its own width and at every wider one; q' = 11 at all five
FITS = [(q, lpl) for q, own in MODULI for lpl in LPLS if lpl >= own]


@pytest.mark.parametrize("q,lpl", FITS, ids=[f"{q.bit_length()}b-{lpl}" for q, lpl in FITS])
def test_quarter_product_bound_at_every_width(q, lpl):
    """acc' < q' + acc f / 2^(29 lpl): with acc < 2 q' and f < 2^87 that is below q' (1 + 2^(88 - 145)) at the narrowest width --
    below 2 q' with room, for the smallest q' as for the widest one the width takes"""
    assert q.bit_length() <= 29 * 4 * lpl - 2
    ring = Ring(q, lpl)
    top = (1 << 63) - 1
    for acc in (0, 1, ring.N - 1, ring.N, 2 * ring.N - 1, ring.one_m):
        for f in (0, 1, 2, ring.N % (1 << 63), top - 1, top, (1 << (3 * W)) - 1):
            r = ring.step(acc, f)
            assert r < ring.N + 1 + (2 * ring.N << (3 * W)) // (1 << (W * lpl)) <= ring.N + 1 + ring.N // (1 << 57)
            assert r * pow(2, W * lpl, ring.N) % ring.N == acc * f % ring.N


@pytest.mark.parametrize("q,lpl", MODULI, ids=IDS)
def test_the_stray_power_cancels_and_the_exponents_are_the_reference(q, lpl):
    ring = Ring(q, lpl)
    lists = [[7], [3, 1], [2, 5, 3], LC.shape_positions(17), list(LC.orders(LC.large_positions(8))["shuffled"])]
    if q == 23:
        lists = [[7], [3, 1], [2, 5, 3], LC.Q23_ON_DEVICE, [1, 2, 3, 4]]
    if q.bit_length() > 2048:                               # (Python's pow of the Fermat power: 0.1 to 0.2 s per coefficient)
        lists = lists[:3]
    for xs in lists:
        m = len(xs)
        stray = pow(2, W * lpl * (m - 1), ring.N)
        for i in range(m):
            num, den = ring.terms(xs, i)
            others = [x for j, x in enumerate(xs) if j != i]
            assert num * stray % ring.N == ring.R * math.prod(others) % ring.N
            assert den * stray % ring.N == ring.R * math.prod(abs(x - xs[i]) for x in others) % ring.N
        flags, exps = ring.exponents(xs)
        assert all(flags) and exps == LC.expected_ints(q, xs), xs


def test_the_check_catches_a_vanishing_denominator_and_leaves_units_alone():
    ring = Ring(23, 5)
    flags, _ = ring.exponents(LC.Q23_VALUE)                 # differences {10, 11}, {10, 1}, {11, 1}: 0 mod 11 for two of the three
    assert flags == [False, True, False]                    # one failed flag sends the WHOLE list to the host
    flags, _ = ring.exponents(LC.Q23_REFUSED)
    assert flags == [False, False]
    flags, exps = ring.exponents(LC.Q23_ON_DEVICE)          # 11 in two numerators: magnitudes 0, one under a negative sign
    assert flags == [True, True, True] and exps == [1, 0, 0] and LC.signs(LC.Q23_ON_DEVICE) == [False, True, False]
    assert exps == LC.expected_ints(23, LC.Q23_ON_DEVICE)


def test_the_check_catches_a_composite_modulus():
    ring = Ring(LC.COMPOSITE_Q, LC.COMPOSITE_LPL)
    for xs in LC.COMPOSITE_LISTS:
        flags, _ = ring.exponents(xs)
        assert not any(flags), xs                           # Fermat's power inverts none of them: the whole list goes to the host
        for i in range(len(xs)):
            assert ring.terms(xs, i)[1] % ring.N == LC.device_denominator(xs, i, ring.N, ring.lpl)
    # and when the check passes the power IS the inverse, whatever the modulus: d x = 1 has one solution x for a unit d
    for d in (1, 2, 2 ** 89, ring.N - 1):
        x = pow(d, -1, ring.N)
        assert ring.product(ring.to_mont_in(x), d) % ring.N == 1


@pytest.mark.parametrize("q,lpl", MODULI, ids=IDS)
def test_store_rule(q, lpl):
    ring = Ring(q, lpl)
    for mag in (0, 1, 2, ring.N - 1):
        if mag >= ring.N:
            continue
        assert ring.store(mag, False) == mag
        v = ring.store(mag, True)
        if mag == 0:
            assert v == 0                                   # the host leaves a magnitude 0 alone under either sign
        else:
            assert v == (q - 1) - mag and v % ring.N == (-mag) % ring.N and ring.N < v < q - 1
            assert v == (-mag) % ring.N + ring.N            # the residue -mag mod q', plus q'


@pytest.mark.parametrize("q,lpl", MODULI[1:], ids=IDS[1:])
def test_product_counts_per_coefficient(q, lpl):
    """2 (m - 1) quarter products; the Fermat power 1 entry + 14 + 4 (nw - 1) + (nw - 1) + 1 full products, nw the 4-bit windows
    of q' - 2; the finish 1 entry + 2.  At 2048 bits and m = 1024: 2 046 quarter products -- the work of (m - 1) / 2 = 511.5 full
    ones -- and 14 + 2 555 + 1 + 2 = 2 572 full ones plus the two entries, against the 2 556 of the share's own power."""
    ring = Ring(q, lpl)
    m = 5
    xs = LC.shape_positions(m)
    num, den = ring.terms(xs, 2)
    assert (ring.quarter, ring.full, ring.entry) == (2 * (m - 1), 0, 0)
    dinv = ring.fermat(den)
    nw = ((ring.N - 2).bit_length() + 3) // 4
    assert (ring.full, ring.entry) == (14 + 5 * (nw - 1) + 1, 1)
    ring.finish(num, den, dinv, False)
    assert (ring.full, ring.entry) == (14 + 5 * (nw - 1) + 1 + 2, 2)
    if q.bit_length() == 2048:
        assert nw == 512 and ring.full + ring.entry == 2574
