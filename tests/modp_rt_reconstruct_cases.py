"""Cases and the reference for `reconstruct` of the run-time MODP groups (mpvss_modp_group_reconstruct) at its shape, modulus and
operand edges: tests/test_gpu_modp_rt_reconstruct_edges.py runs them on the GPU, tests/test_modp_rt_reconstruct_cases.py holds
them to the oracle.  The reference is ref_reconstruct of tests/reconstruct_cases.py over RtOracleGroup(q): exact Fraction
coefficients (a Fraction is in lowest terms, as participant.rs:546-553 makes num / den before it inverts den), the magnitude mod
q' = (q-1)/2, pow, element_inverse for a negative coefficient, REFUSED where the reduced denominator has no inverse mod q'.

Honest shares are powers of the subgroup generator g = 4 with the polynomial over Z/q': 4 has order q' for every safe prime, so
the ("identity", s) expectation is 4^P(0) also where 2 is a non-residue (q = 3 mod 8).  `power(base, exps)` makes them: the
handle's fixed-base call on the GPU, Python's pow on the CPU.

Builder of tests/reconstruct_cases.py is inherited, not copied: the seeded polynomials, shape_case, position_cases, sign_positions
and sign_lanes are its own."""
import functools
import itertools
import random

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import mpvss_oracle as O
from reconstruct_cases import (Builder, Case, REFUSED, exact_lagrange, lane_signs, large_positions, orders, ref_reconstruct,  # noqa: F401
                               synthetic_box)

# key -> (modulus, bytes of an element on the ABI, limbs per lane the handle runs at)
GROUPS = {
    "q23": (lambda: 23, 256, 5),
    "q47": (lambda: 47, 256, 5),
    "b40": (lambda: H.small_safe_primes()[40], 256, 5),           # 7 mod 8
    "b64": (lambda: H.small_safe_primes()[64], 256, 5),           # 3 mod 8: 2 is a non-residue
    "b256": (lambda: H.small_safe_primes()[256], 256, 5),
    "rfc1024": (lambda: H.rfc_prime(1024), 256, 9),
    "rfc2048": (lambda: H.rfc_prime(2048), 256, 18),
    "rfc3072": (WH.group15, WH.EB, WH.LPL),
}
KEYS = tuple(GROUPS)
WIDTHS = ("b40", "rfc1024", "rfc2048", "rfc3072")                 # one handle per limb width: 5, 9, 18, 27
# family A: every parity pattern of the pairwise fold up to three levels (1..9), the odd element carried across more levels
# (15..65, 255..257), powers of two and their neighbours; 4097 is the ragged last workgroup of the launches, at 40 bits only
SHAPE_M = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]
SHAPE_M_BIG = 4097
POSITION_KEYS = ("b40", "b64", "b256", "rfc2048", "rfc3072")
POSITION_M = [17, 65]
SMALL_Q = ("b40", "b64")                                          # q' below 2^63: positions reach and pass it
SIGN_KEYS = ("b64", "b256", "rfc1024", "rfc2048", "rfc3072")
SIGN_M = [5, 17]
DEVICE_KEYS = ("b40", "rfc2048", "rfc3072")
DEVICE_M = [1, 65, 257]
MASK_KEYS = SMALL_Q + ("b256",)
# family C: every position set of these sizes out of 1..top, against the oracle itself
TINY = {"q23": (14, 4), "q47": (26, 3)}
# what the reference gives on them: (sets, a value, None, a value although a raw denominator is 0 mod q')
TINY_COUNTS = {"q23": (1470, 1272, 198, 36), "q47": (2951, 2879, 72, 3)}
Q_1_MOD_4 = 1000000009                                            # a prime with (q-1)/2 even: the documented limit of the call


class RtGroup(H.RtOracleGroup):
    """RtOracleGroup with the handle's element width at the fixed-width boundary"""

    def __init__(self, q, eb):
        super().__init__(q)
        self.eb = self.elem_len = self.scalar_len = eb

    def element_to_fixed(self, e):
        return e.to_bytes(self.eb, "big")

    def scalar_to_fixed(self, s):
        return s.to_bytes(self.eb, "big")


@functools.lru_cache(maxsize=None)
def modulus(key):
    return GROUPS[key][0]()


def python_power(key):
    """the CPU module's maker of honest shares: pow, and above 512 bits (where a pow of Python costs 20 .. 70 ms and the module makes
    hundreds) one product per 4-bit digit of the exponent over the powers base^(d 16^i).  ref_reconstruct never comes here: it
    checks these shares with pow."""
    q, eb = modulus(key), GROUPS[key][1]
    rows = {}

    def power(base, exps):
        if q.bit_length() <= 512:
            return [pow(base, e, q).to_bytes(eb, "big") for e in exps]
        if base not in rows:
            rows[base], b = [], base
            for _ in range((q.bit_length() + 3) // 4):
                row = [1]
                for _ in range(15):
                    row.append(row[-1] * b % q)
                rows[base].append(row)
                b = row[15] * b % q
        out = []
        for e in exps:
            acc, i = 1, 0
            while e:
                acc, e, i = acc * rows[base][i][e & 15] % q, e >> 4, i + 1
            out.append(acc.to_bytes(eb, "big"))
        return out

    return power


def raw_denominator_vanishes(positions, sub):
    """some prod_{j != i} (x_j - x_i) is 0 mod q' before the fraction is reduced"""
    return any(any((x - xi) % sub == 0 for x in positions if x != xi) for xi in positions)


class RtBuilder(Builder):
    def __init__(self, key, power=None):
        self.name = key
        self.q, self.EB, self.lpl = modulus(key), GROUPS[key][1], GROUPS[key][2]
        self.G = RtGroup(self.q, self.EB)
        self.sub = (self.q - 1) // 2
        self.ring = self.sub                                # the polynomial lives in Z/q', the exponents of g = 4
        self._power_of = power or python_power(key)
        self._power = lambda exps: self._power_of(4, exps)
        self._made = {}
        self._made2 = {}

    def fix(self, v):
        return v.to_bytes(self.EB, "big")

    def shape_sizes(self, limit):
        """sizes of family A at which positions 1..m stay different mod q' (only the two tiny moduli lose any)"""
        return [m for m in SHAPE_M if m <= limit and m < self.sub]

    # ---- B2: positions at and past q' ----------------------------------------------------------------------------------
    def small_q_cases(self):
        """what the reduced fraction decides: a list of [Case] groups; the cases of a group must give the same bytes"""
        s = self.sub
        coeffs = self.poly(2, 3500)

        def case(tag, xs, kind):
            return Case(f"B2-{tag}", xs, self.power(self.values(coeffs, xs)), (kind, None))

        out = [[case("two-congruent", [1, 1 + s], "refuse")],
               [case("four-congruent", [2, 2 + s, 5, 7], "refuse")],
               # lambda of 1 is q' (1 + q') / ((q' - 1) q'): the raw denominator is 0 mod q', the reduced one is not
               [case(f"gcd-{o}", xs, "ref") for o, xs in orders([s, 1, 1 + s]).items()]]
        if 2 * s < 2 ** 63:                                  # (2 q' = q - 1 of the 64-bit prime is no int64)
            out.append([case("numerator-q2", [s, 2 * s, 3], "ref")])      # q' twice in a numerator, once in a denominator
        return out

    # ---- C: every small set at a tiny modulus --------------------------------------------------------------------------
    def tiny_cases(self):
        top, kmax = TINY[self.name]
        coeffs = self.poly(3, 8000)
        share = dict(zip(range(1, top + 1), self.power(self.values(coeffs, range(1, top + 1)))))
        out = []
        for k in range(1, kmax + 1):
            for combo in itertools.combinations(range(1, top + 1), k):
                xs = list(combo)
                random.Random(len(out)).shuffle(xs)
                out.append(Case(f"C-{'-'.join(map(str, combo))}", xs, [share[x] for x in xs], ("oracle", None)))
        return out

    # ---- D: signs and degenerate shares --------------------------------------------------------------------------------
    def power2(self, exps):
        """encodings of G^e for the main generator G = 2"""
        todo = [e for e in dict.fromkeys(exps) if e not in self._made2]
        for e, enc in zip(todo, self._power_of(2, todo)):
            self._made2[e] = enc
        return [self._made2[e] for e in exps]

    def sign_cases(self, m):
        """the fixed MODP family's cases at the handle's width"""
        q, fix, xs = self.q, self.fix, self.sign_positions(m)
        base, _ = self.dealt(xs, 4, 5000 + m)
        (p0, p1), (n0, n1) = self.sign_lanes(xs)
        top = 2 ** (8 * self.EB) - 1

        def put(*pairs):
            sh = list(base)
            for lane, enc in pairs:
                sh[lane] = enc
            return sh

        S = self.power([self.poly(1, 6000 + m)[0]])[0]
        cases = [
            Case(f"D-m{m}-equal", xs, [S] * m, ("ref", S)),                           # the coefficients sum to 1
            Case(f"D-m{m}-all-one", xs, [fix(1)] * m, ("ref", fix(1))),
            Case(f"D-m{m}-swapped", xs, put((p0, base[n0]), (n0, base[p0])), ("ref", None)),
            Case(f"D-m{m}-minus-one-pos", xs, put((p0, fix(q - 1)), (n0, fix(1))), ("ref", None)),   # q - 1: a non-residue
            Case(f"D-m{m}-minus-one-neg", xs, put((n0, fix(q - 1)), (p0, fix(1))), ("ref", None)),
            Case(f"D-m{m}-unreduced", xs, put((p0, fix(top)), (n0, fix(q + 5))), ("ref", None)),
            Case(f"D-m{m}-unreduced-swapped", xs, put((n1, fix(top)), (p1, fix(q + 5))), ("ref", None)),
            Case(f"D-m{m}-zero-pos", xs, put((p1, fix(0))), ("ref", fix(0))),
            Case(f"D-m{m}-q-pos", xs, put((p1, fix(q))), ("ref", fix(0))),
            Case(f"D-m{m}-zero-neg", xs, put((n1, fix(0))), ("refuse", None)),
            Case(f"D-m{m}-q-neg", xs, put((n1, fix(q))), ("refuse", None)),
        ]
        if self.name == "b64":
            # honest shares of G = 2, which has order q - 1 here: the polynomial over Z/(q-1), the coefficients still mod q', so
            # the result is G^s or -G^s -- the reference says which
            rng = random.Random(6500 + m)
            coeffs = [rng.randrange(q - 1) for _ in range(4)]
            vals = [sum(a * x ** k for k, a in enumerate(coeffs)) % (q - 1) for x in xs]
            cases.append(Case(f"D-m{m}-main-generator", xs, self.power2(vals), ("ref", None)))
        return cases

    # ---- E: the mask's reduction mod q ---------------------------------------------------------------------------------
    def mask_cases(self, count=8):
        """seeded m = 3 cases; at 256 bits the hashes of their results fall on both sides of q"""
        out = []
        for k in range(count):
            xs = [2, 3, 1]
            shares, s = self.dealt(xs, 3, 9000 + k)
            out.append(Case(f"E-mask-{k}", xs, shares, ("identity", s)))
        return out

    def refused_arguments(self):
        """(positions, shares) that the call refuses before it computes: duplicates at the two ends of an m = 257 list, position
        0 or -1 on each of 3 lanes, m = 0"""
        big = self.shape_case(257)
        dup = list(big.positions)
        dup[-1] = dup[0]
        three = self.shape_case(3)
        bad = [(dup, big.shares)]
        for x in (0, -1):
            for lane in range(3):
                xs = list(three.positions)
                xs[lane] = x
                bad.append((xs, three.shares))
        bad.append(([], []))
        return bad

    # ---- what a case expects -------------------------------------------------------------------------------------------
    def reference(self, case, memo=None):
        """ref_reconstruct as an encoding, or None where the reference returns None"""
        r = ref_reconstruct(self.G, case.positions, self.elements(case), memo)
        return None if r is REFUSED else self.fix(r)

    def expected(self, case, memo=None):
        """the encoding of G^s that the case expects, or None for a refusal"""
        kind, v = case.expect
        if kind == "identity":
            return self.fix(pow(4, v, self.q))
        if kind == "refuse":
            return None
        if kind == "oracle":
            return self.reference(case, memo)
        return super().expected(case, memo)

    def hash_below_q(self, gs_enc):
        """whether int(SHA-256(minimal bytes of G^s)) is below q, so that the mask's reduction leaves it alone"""
        return int.from_bytes(O.sha256(self.G.element_to_bytes(self.G.element_from_fixed(gs_enc))), "big") < self.q


def interleaved_order():
    """(key, m) of family A's mixed pass.  Four descending runs over SHAPE_M with the handle changing at every call, each run
    starting at another width: every size below 257 runs at every width right after a larger call of another width.  Then one zigzag,
    largest, smallest, second largest, ...: a small call after a much larger one of another width, and a large one after a
    small one."""
    out = []
    down = SHAPE_M[::-1]
    for start in range(len(WIDTHS)):
        out += [(WIDTHS[(start + 3 * k) % len(WIDTHS)], m) for k, m in enumerate(down)]
    zig = [m for pair in zip(down, SHAPE_M) for m in pair][:len(down)]
    out += [(WIDTHS[(3 * k) % len(WIDTHS)], m) for k, m in enumerate(zig)]
    return out
