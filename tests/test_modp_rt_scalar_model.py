"""Integer model of the scalar-ring kernels of a run-time MODP group (k_rt_modq_mul, k_rt_modq_responses, k_rt_modq_poly_eval in
mpvss_rs_amd/csrc/modp_rt_kernels.inc): Z/(q-1) = Z/2 x Z/q' for odd q' = (q-1)/2, residues mod q' in Montgomery form with the lazy
[0, 2N) product at the handle's own width (L = 20, 36, 72, 108 limbs of 29 bits), parities on the side, lifted when written.

The model is exact integers: a product of `rows` rows is (a b + m N) / 2^(29 rows) with m = -a b / N mod 2^(29 rows), which is
what the CIOS loop of bn::mont_mul computes, below N + a b / 2^(29 rows).  It asserts the bounds the kernels rely on, the lifting
rule, the results against Python integers, and the operation counts.  No library, no GPU."""
import random

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH

W = 29


def geometry(q, wide=False):
    lpl = 27 if wide else H.width_for_bits(q.bit_length())
    eb = 384 if wide else 256
    L = 4 * lpl
    in_rows = lpl * (((8 * eb + 28) // 29 + lpl - 1) // lpl)
    return L, eb, in_rows


class Ring:
    """the constants of q' the handle builds (n, kin, one_m, one) and the three kernels"""

    def __init__(self, q, wide=False):
        assert q % 4 == 3 and q >= 7
        self.q, self.N = q, (q - 1) // 2
        self.L, self.EB, self.IN_ROWS = geometry(q, wide)
        self.R = 1 << (W * self.L)
        assert self.R > 8 * self.N                      # q' has one bit fewer than q, and R > 4 q
        self.kin = pow(2, W * (self.IN_ROWS + self.L), self.N)
        self.one_m = self.R % self.N
        self.products = 0

    def mont(self, a, b, rows=None, a_bound=None):
        rows = self.L if rows is None else rows
        Rr = 1 << (W * rows)
        if a_bound is not None:
            assert a < a_bound
        m = (-a * b * pow(self.N, -1, Rr)) % Rr
        t, rem = divmod(a * b + m * self.N, Rr)
        assert rem == 0 and t < self.N + a * b // Rr + 1
        self.products += 1
        return t

    def to_mont_in(self, x):
        """any EB-byte input -> x R mod q', below 2 q'"""
        assert 0 <= x < 1 << (8 * self.EB) <= 1 << (W * self.IN_ROWS)
        r = self.mont(self.kin, x, self.IN_ROWS)
        assert r < 2 * self.N and r % self.N == x * self.R % self.N
        return r

    def lift(self, almost, parity):
        """store_canonical_lift: canonical residue, plus q' when its low bit is not the wanted parity"""
        assert almost < 2 * self.N
        v = almost - self.N if almost >= self.N else almost
        if (v & 1) != parity:
            v += self.N
        assert 0 <= v < self.q - 1 and (v & 1) == parity
        return v

    def mul(self, a, b):
        parity = a & b & 1
        ar = self.to_mont_in(a)
        br = self.to_mont_in(b)
        acc = self.mont(ar, br, a_bound=2 * self.N)
        acc = self.mont(acc, 1, a_bound=2 * self.N)
        return self.lift(acc, parity)

    def responses(self, w, alpha, c):
        c %= self.q - 1
        cneg, c_parity = (-c) % self.N, c & 1             # what the host passes
        parity = (w ^ (alpha & c_parity)) & 1
        acc = self.to_mont_in(cneg)
        v = self.to_mont_in(alpha)
        acc = self.mont(acc, v, a_bound=2 * self.N)
        assert acc < 2 * self.N
        v = self.to_mont_in(w)
        acc += v
        assert acc < 4 * self.N < self.R
        acc = self.mont(acc, 1, a_bound=4 * self.N)
        return self.lift(acc, parity)

    def stage(self, coeffs):
        """the host's staging: (a_j mod q') R mod q' canonical, and the two parities"""
        red = [a % (self.q - 1) for a in coeffs]
        par_even, par_odd = red[0] & 1, 0
        for a in red:
            par_odd ^= a & 1
        return [a % self.N * self.one_m % self.N for a in red], par_even, par_odd

    def poly_eval(self, staged, pos):
        coef, par_even, par_odd = staged
        assert 0 <= pos < 1 << 63
        pr = self.mont(self.kin, pos, self.IN_ROWS)       # three limbs of the position, zeros above
        assert pr < 2 * self.N
        acc = coef[-1]
        for j in range(len(coef) - 2, -1, -1):
            acc = self.mont(acc, pr, a_bound=4 * self.N)  # the product's input bound: 4 q' 2 q' / R < q'
            assert acc < 2 * self.N
            acc += coef[j]
            assert acc < 4 * self.N
        acc = self.mont(acc, 1, a_bound=4 * self.N)
        return self.lift(acc, par_odd if pos & 1 else par_even)


def _moduli():
    sp = H.small_safe_primes()
    return [(7, False), (23, False), (sp[40], False), (sp[512], False), (H.rfc_prime(1024), False), (H.rfc_prime(2048), False),
            (WH.group15(), True)]


MODULI = _moduli()
IDS = [f"{q.bit_length()}b" for q, _ in MODULI]


def operands(ring, rng, extra=3):
    q, top = ring.q, (1 << (8 * ring.EB)) - 1
    ops = [0, 1, ring.N - 1, ring.N, q - 2, q - 1, q, top]
    ops += [rng.randrange(q) for _ in range(extra)] + [rng.randrange(top + 1) for _ in range(extra)]
    return ops


def test_widths_are_the_four_instantiated_ones():
    assert sorted({geometry(q, w)[0] for q, w in MODULI}) == [20, 36, 72, 108]
    assert [geometry(q, w)[2] for q, w in MODULI[3:]] == [75, 72, 72, 108]


@pytest.mark.parametrize("q,wide", MODULI, ids=IDS)
def test_entry_bound_for_an_all_ones_input(q, wide):
    ring = Ring(q, wide)
    top = (1 << (8 * ring.EB)) - 1
    assert ring.to_mont_in(top) < 2 * ring.N                # asserted inside as well, for every input


@pytest.mark.parametrize("q,wide", MODULI, ids=IDS)
def test_lifting_gives_the_value_mod_q_minus_1(q, wide):
    ring = Ring(q, wide)
    for residue in (0, ring.N - 1):
        for parity in (0, 1):
            for almost in (residue, residue + ring.N):      # both forms of an almost-normalised residue
                v = ring.lift(almost, parity)
                assert v % ring.N == residue and v % 2 == parity and 0 <= v < q - 1
                # the unique such value: Chinese remainders over 2 and the odd q'
                assert [x for x in (residue, residue + ring.N) if x % 2 == parity] == [v]


@pytest.mark.parametrize("q,wide", MODULI, ids=IDS)
def test_mul_and_its_count(q, wide):
    ring = Ring(q, wide)
    ops = operands(ring, random.Random(q & 0xFFFF))
    for a in ops:
        for b in ops:
            before = ring.products
            assert ring.mul(a, b) == a * b % (q - 1), (a, b)
            assert ring.products - before == 4              # two entries, the product, the exit


@pytest.mark.parametrize("q,wide", MODULI, ids=IDS)
def test_responses_and_their_count(q, wide):
    ring = Ring(q, wide)
    rng = random.Random(q & 0xFFFFF)
    ops = operands(ring, rng, extra=2)
    for c in (0, ring.N, q - 2, rng.randrange(ring.N), (1 << (8 * ring.EB)) - 1):
        for w in ops:
            for alpha in ops:
                before = ring.products
                assert ring.responses(w, alpha, c) == (w - alpha * c) % (q - 1), (w, alpha, c)
                assert ring.products - before == 5          # three entries, the product, the exit


@pytest.mark.parametrize("q,wide", MODULI, ids=IDS)
@pytest.mark.parametrize("t", [1, 2, 3, 17])
def test_poly_eval_and_its_count(q, wide, t):
    ring = Ring(q, wide)
    rng = random.Random(t * 131 + (q & 0xFFF))
    ops = operands(ring, rng)
    for trial in range(3):
        coeffs = [ops[(trial * t + j) % len(ops)] if trial < 2 else rng.randrange(1 << (8 * ring.EB)) for j in range(t)]
        staged = ring.stage(coeffs)
        assert all(c < ring.N for c in staged[0])
        for pos in [0, 1, 2, 1 << 31, (1 << 63) - 1] + list(range(5, 9)) + [rng.randrange(1 << 63)]:
            before = ring.products
            want = sum(a * pos ** j for j, a in enumerate(coeffs)) % (q - 1)
            assert ring.poly_eval(staged, pos) == want, (coeffs, pos)
            assert ring.products - before == (t - 1) + 2    # Horner, the position's entry, the exit


def test_horner_accumulator_bound_is_reached_from_the_worst_inputs():
    """acc' < (q' + acc 2q'/R) + q': with acc < 4 q' and R > 8 q' that is below 3 q' -- the 4 q' the kernel allows is never passed,
    for the largest staged coefficients and the largest product operand the entry can give"""
    for q, wide in MODULI:
        ring = Ring(q, wide)
        worst_b = 2 * ring.N - 1
        acc = 4 * ring.N - 1
        for _ in range(4):
            acc = ring.mont(acc, worst_b, a_bound=4 * ring.N) + (ring.N - 1)
            assert acc < 3 * ring.N
