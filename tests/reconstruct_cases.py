"""Cases and the reference for `reconstruct` of the three fixed groups at its shape and operand edges
(tests/test_gpu_reconstruct_edges.py runs them on the GPU, tests/test_reconstruct_cases.py holds them to the oracle).

The reference, ref_reconstruct, shares nothing with the engine: exact Lagrange coefficients at 0 as fractions.Fraction over
Python integers, the magnitude |num| |den|^-1 mod the subgroup order (MODP) or the group order (curves), G.exp on the oracle's
group, G.element_inverse for a negative coefficient (participant.rs:551-553, 1546-1555), the fold with G.mul.

A case is (positions, shares, expectation).  Shares are fixed-width encodings; most are G^P(i) for a polynomial the builder
knows, made by `power`, a function from exponents to encodings: the engine's fixed-base calls on the GPU, the oracle on the CPU.
The expectation is one of
  ("identity", s)   G^s with s = P(0): the polynomial identity, no exponentiation per share on the CPU
  ("ref", claim)    ref_reconstruct; claim is None or an encoding that the builder says the result has
  ("refuse", None)  the call fails (MODP: a share that is 0 mod q where its factor has to be inverted)"""
import math
import random
from collections import namedtuple
from fractions import Fraction

import mpvss_oracle as O
from helpers import modp_keygen

NAMES = ("modp2048", "secp256k1", "ristretto255")
CURVES = NAMES[1:]
T_SHAPE = 8
# family A.  Curves: the wave and workgroup edges of the one-workgroup sum (64 lanes a wave, 256 lanes, the second and third pass
# of its stride loop) and the edge of the validity flags' sizing rule (4096).  MODP: every parity pattern of the pairwise fold
# and the switch from the row to the quad layout (4096).  The two largest sizes pay the host's quadratic Lagrange loop and run
# in a test of their own.
SHAPE_M = {
    "modp2048": list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 255, 256, 257],
    "secp256k1": [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513],
    "ristretto255": [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513],
}
SHAPE_M_BIG = [4096, 4097]
DEVICE_M = [1, 65, 257]
# family B: the ends of int64 and the 32-bit edges; `position as u64` multiplies into the numerator, the signed difference of
# two positions into the denominator (both below 2^63 in magnitude for positions in [1, 2^63 - 1])
SPECIAL = [2 ** 63 - 1, 1, 2 ** 32, 2 ** 63 - 2, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 61 - 1]
POSITION_M = [17, 65]
SIGN_M = [5, 17]
LANES_257 = [0, 63, 64, 255, 256]

Case = namedtuple("Case", "id positions shares expect")
REFUSED = "refused"       # what ref_reconstruct returns where the reference returns None (None itself is secp256k1's identity)


def lagrange_modulus(G):
    """what the coefficients are reduced by: (q-1)/2 (participant.rs:540-548) or the curve's order (:1518-1544, 1955-1990)"""
    return G.subgroup_order() if G.name == "modp2048" else G.group_order_int()


def product(v):
    """of a list of integers, by chunks: the partial products stay balanced (a running product costs four times as much at
    m = 4097)"""
    while len(v) > 1:
        v = [math.prod(v[k:k + 8]) for k in range(0, len(v), 8)]
    return v[0] if v else 1


def exact_lagrange(positions):
    """lambda_i = prod_{j != i} x_j / (x_j - x_i), exact"""
    xs = list(positions)
    if len(set(xs)) != len(xs):
        raise ValueError("duplicate positions")
    whole = product(xs)
    out = []
    for i, xi in enumerate(xs):
        diffs = [x - xi for x in xs]
        del diffs[i]
        out.append(Fraction(whole // xi, product(diffs)))          # (positions are >= 1: the division is exact)
    return out


def lane_signs(positions):
    """the builder's claim: lambda_i < 0 exactly when an odd number of positions lie below x_i (every such x_j - x_i is a
    negative factor of the denominator, the numerator is positive) -- in whatever order the positions come"""
    rank = {x: r for r, x in enumerate(sorted(positions))}
    return [rank[x] & 1 == 1 for x in positions]


def ref_reconstruct(G, positions, shares, memo=None):
    """G^s from oracle elements `shares` at `positions`, or REFUSED where the reference returns None (MODP: a factor without
    inverse).  memo: (share, magnitude, negative) -> factor, for callers whose cases share factors."""
    mod = lagrange_modulus(G)
    acc = G.identity()
    for lam, S in zip(exact_lagrange(positions), shares):
        try:
            mag = abs(lam.numerator) * pow(lam.denominator, -1, mod) % mod
        except ValueError:            # the denominator in lowest terms has no inverse (a run-time group with a small (q-1)/2)
            return REFUSED
        key = (S, mag, lam < 0)
        if memo is not None and key in memo:
            f = memo[key]
        else:
            f = G.exp(S, mag)
            if lam < 0:
                f = G.element_inverse(f)
            if memo is not None:
                memo[key] = f
        if f is None and G.identity() is not None:        # (None is secp256k1's identity, not a failure)
            return REFUSED
        acc = G.mul(acc, f)
    return acc


def oracle_power(G):
    """exponents -> encodings of G^e by the oracle (the CPU module; the GPU module passes the engine's fixed-base calls)"""
    return lambda exps: [G.element_to_fixed(G.exp(G.generator(), e)) for e in exps]


def large_positions(m, seed=5):
    """ascending: the first m of SPECIAL, then seeded values below 2^62"""
    rng = random.Random(seed)
    xs = set(SPECIAL[:m])
    while len(xs) < m:
        xs.add(rng.randrange(2, 2 ** 62))
    return sorted(xs)


def orders(xs, seed=9):
    sh = list(xs)
    random.Random(seed).shuffle(sh)
    return {"asc": sorted(xs), "desc": sorted(xs, reverse=True), "shuffled": sh}


class Builder:
    def __init__(self, name, power=None):
        self.name = name
        self.G = O.GROUPS[name]()
        self.ring = self.G.group_order_int()                # P(i) mod q-1 (participant.rs:202) / mod the curve's order
        self._power = power or oracle_power(self.G)
        self._made = {}

    # ---- shares ------------------------------------------------------------------------------------------------------
    def power(self, exps):
        todo = [e for e in dict.fromkeys(exps) if e not in self._made]
        if todo:
            for e, enc in zip(todo, self._power(todo)):
                self._made[e] = enc
        return [self._made[e] for e in exps]

    def poly(self, t, seed):
        rng = random.Random(seed)
        return [rng.randrange(self.ring) for _ in range(t)]

    def values(self, coeffs, positions):
        out = []
        for x in positions:
            acc = 0
            for a in reversed(coeffs):
                acc = (acc * x + a) % self.ring
            out.append(acc)
        return out

    def dealt(self, positions, t, seed):
        """(shares G^P(i), P(0)) of a seeded polynomial with t coefficients"""
        coeffs = self.poly(t, seed)
        return self.power(self.values(coeffs, positions)), coeffs[0]

    def identity_enc(self):
        return self.G.element_to_fixed(self.G.identity())

    # ---- A: shape ----------------------------------------------------------------------------------------------------
    def shape_positions(self, m):
        xs = list(range(1, m + 1))
        random.Random(1000 + m).shuffle(xs)
        return xs

    def shape_case(self, m):
        xs = self.shape_positions(m)
        shares, s = self.dealt(xs, min(T_SHAPE, m), 2000 + m)       # (m shares determine a polynomial of at most m coefficients)
        return Case(f"A-m{m}", xs, shares, ("identity", s))

    # ---- B: positions ------------------------------------------------------------------------------------------------
    def position_cases(self, m, t=T_SHAPE):
        """the same shares in three orders: {order: Case}, every one G^P(0)"""
        out = {}
        coeffs = self.poly(t, 3000 + m)
        for order, xs in orders(large_positions(m)).items():
            out[order] = Case(f"B-m{m}-{order}", xs, self.power(self.values(coeffs, xs)), ("identity", coeffs[0]))
        return out

    # ---- C: signs and degenerate shares ------------------------------------------------------------------------------
    def sign_positions(self, m):
        """unsorted, small enough for the oracle's MODP loop over 1..max (util.rs:47-64)"""
        return random.Random(4000 + m).sample(range(1, 41), m)

    def sign_lanes(self, xs):
        """(two lanes with a positive coefficient, two with a negative one)"""
        neg = lane_signs(xs)
        pos_l = [k for k in range(len(xs)) if not neg[k]]
        neg_l = [k for k in range(len(xs)) if neg[k]]
        return pos_l[-2:], neg_l[-2:]

    def sign_cases(self, m):
        G, xs = self.G, self.sign_positions(m)
        base, _ = self.dealt(xs, 4, 5000 + m)
        (p0, p1), (n0, n1) = self.sign_lanes(xs)
        ident = self.identity_enc()

        def put(*pairs):
            sh = list(base)
            for lane, enc in pairs:
                sh[lane] = enc
            return sh

        S = self.power([self.poly(1, 6000 + m)[0]])[0]
        swapped = put((p0, base[n0]), (n0, base[p0]))
        cases = [Case(f"C-m{m}-equal", xs, [S] * m, ("ref", S)),                      # sum of the coefficients is 1
                 Case(f"C-m{m}-all-identity", xs, [ident] * m, ("ref", ident)),
                 Case(f"C-m{m}-swapped", xs, swapped, ("ref", None))]
        if self.name == "modp2048":
            q = G.q
            fix = lambda v: v.to_bytes(256, "big")
            cases += [
                Case(f"C-m{m}-minus-one-pos", xs, put((p0, fix(q - 1)), (n0, fix(1))), ("ref", None)),     # q - 1: a non-residue
                Case(f"C-m{m}-minus-one-neg", xs, put((n0, fix(q - 1)), (p0, fix(1))), ("ref", None)),
                Case(f"C-m{m}-unreduced", xs, put((p0, fix(2 ** 2048 - 1)), (n0, fix(q + 5))), ("ref", None)),
                Case(f"C-m{m}-unreduced-swapped", xs, put((n1, fix(2 ** 2048 - 1)), (p1, fix(q + 5))), ("ref", None)),
                Case(f"C-m{m}-zero-pos", xs, put((p1, fix(0))), ("ref", fix(0))),
                Case(f"C-m{m}-q-pos", xs, put((p1, fix(q))), ("ref", fix(0))),
                Case(f"C-m{m}-zero-neg", xs, put((n1, fix(0))), ("refuse", None)),
                Case(f"C-m{m}-q-neg", xs, put((n1, fix(q))), ("refuse", None)),
            ]
        else:
            vals = self.values(self.poly(4, 5000 + m), xs)
            minus = self.power([(self.ring - vals[p0]) % self.ring])[0]                 # -S of lane p0
            lo = min(p1, m - 2)
            cases += [
                Case(f"C-m{m}-identity-pos", xs, put((p0, ident)), ("ref", None)),
                Case(f"C-m{m}-identity-neg", xs, put((n0, ident)), ("ref", None)),
                Case(f"C-m{m}-negated", xs, put((n0, minus)), ("ref", None)),           # S_n0 = -S_p0
                Case(f"C-m{m}-adjacent-equal", xs, put((lo + 1, base[lo])), ("ref", None)),
            ]
        return cases

    def lane_case_257(self, lane):
        """curves: the identity on one lane of m = 257 (lane 256 is lane 0's second pass of the stride loop)"""
        xs = self.shape_positions(257)
        shares, _ = self.dealt(xs, T_SHAPE, 2000 + 257)
        shares = list(shares)
        shares[lane] = self.identity_enc()
        return Case(f"C-m257-identity-lane{lane}", xs, shares, ("ref", None))

    # ---- what a case expects -----------------------------------------------------------------------------------------
    def elements(self, case):
        return [self.G.element_from_fixed(s) for s in case.shares]

    def expected(self, case, memo=None):
        """the encoding of G^s that the case expects, or None for a refusal"""
        kind, v = case.expect
        if kind == "identity":
            return self.G.element_to_fixed(self.G.exp(self.G.generator(), v))
        if kind == "refuse":
            return None
        r = ref_reconstruct(self.G, case.positions, self.elements(case), memo)
        assert r is not REFUSED, case.id
        enc = self.G.element_to_fixed(r)
        assert v is None or enc == v, case.id
        return enc

    def mask(self, gs_enc):
        """the 32-byte mask of an encoded G^s (participant.rs:512-517, 1495-1511, 1939-1949)"""
        return self.G.secret_mask(self.G.element_from_fixed(gs_enc)).to_bytes(32, "big")


def gpu_position_lists(name):
    """every position list that tests/test_gpu_reconstruct_edges.py sends to the engine for this group, refusals aside"""
    b = Builder(name, power=lambda exps: [b""] * len(exps))
    lists = [b.shape_positions(m) for m in SHAPE_M[name] + SHAPE_M_BIG]
    for m in POSITION_M:
        lists += list(orders(large_positions(m)).values())
    lists += [b.sign_positions(m) for m in SIGN_M]
    lists += [[3, 1, 2]]                                   # the call after a refusal
    return lists


def dealt_instance(name, n, t, seed, secret):
    """a really dealt box with its decrypted shares, all by the oracle"""
    G = O.GROUPS[name]()
    rng = random.Random(seed)
    order = G.group_order_int()
    keygen = (lambda: modp_keygen(G, rng)) if name == "modp2048" else (lambda: rng.randrange(1, order))
    privs = [keygen() for _ in range(n)]
    wits = [keygen() for _ in range(2 * n)]
    pks = [G.generate_public_key(k) for k in privs]
    coeffs = [rng.randrange(order) for _ in range(t)]
    box = O.distribute_secret(G, secret, pks, t, coeffs, wits[:n])
    sbs = [O.extract_secret_share(G, box, k, w) for k, w in zip(privs, wits[n:])]
    return G, pks, box, sbs


def synthetic_box(G, case):
    """(shareboxes, box) for O.reconstruct: any distinct public keys mapped to the case's positions, U = 0, one dummy commitment"""
    if G.name == "modp2048":
        pks = list(range(2, 2 + len(case.positions)))
    else:
        pks, P = [], G.generator()
        for _ in case.positions:
            pks.append(P)
            P = G.mul(P, G.generator())
    box = {"commitments": [G.generator()], "positions": {G.element_to_bytes(pk): x for pk, x in zip(pks, case.positions)}, "U": 0}
    sbs = [{"publickey": pk, "share": G.element_from_fixed(s)} for pk, s in zip(pks, case.shares)]
    return sbs, box
