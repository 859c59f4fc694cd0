"""Child process of tests/test_gpu_modp_rt_fd_edges.py: the forward-difference X path of the run-time MODP groups
(k_rt_commit_eval_mont, k_rt_fd_chain, k_rt_from_mont behind rt_commit_eval_dev, rt_fd_prepare and rt_fd_positions_ok; DESIGN
section 13) at its edges.  One child runs every case of ONE width (limbs per lane) on one context and prints one line per case:

    case <case id> <sha256 of the mode-2 bytes> <path>

    python modp_rt_fd_edge_child.py 5 | 9 | 18 | 27 | chunks          (chunks: with MPVSS_MAX_CHUNK=64 in the environment)

and `modp rt fd edges <width> ok` as its last line; it exits non-zero at the first mismatch, naming the case.

Families (build_cases): A degenerate commitments -- the Montgomery one, q - 1, equal and inverse commitments, values >= q -- as
difference levels; B roots inside the run (X = 1 at a chain's edge, at a seed, next to a seed); C shapes: t around every wave
boundary up to the largest workgroup, chains with no steps, with steps in one direction only, ragged, thousands of steps, 64
chains of two seeds; D first positions up to 2^63 - n, around q - 1 and below zero; E state kept in the context between calls
(run in order, after the cases, on the same context); F whole boxes whose polynomial has zero coefficients.

Every case runs under mode 2 (forward differences whenever admissible) with the case's `chains` and under mode 0 (Horner's
rule): the bytes must be equal at ALL positions, mpvss_modp_group_fd_stats must show the expected path, and both are compared
with Python integers -- Horner's rule in the exponent for units, prod_j C_j^(i^j mod (q-1)) where a commitment is no unit -- at
the positions the case fixes (Case.at): all of them when q has at most 640 bits and n t <= 8192, otherwise every chain's first
and last position, first and last seed, the position next to the seeds on either side, and every planted root.

build_cases() needs neither torch nor a GPU: tests/test_modp_rt_fd_edge_cases.py checks the cases against the integer model."""
import functools
import hashlib
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import modp_rt_helpers as H  # noqa: E402
import modp_rt_wide_helpers as WH  # noqa: E402

WIDTHS = ("5", "9", "18", "27")
FD_MAX_T = {5: 256, 9: 256, 18: 256, 27: 128}       # MODP_RT_FD_MAX_T (modp_rt_kernels.h); the child asserts the handles say the same
ALL_BITS, ALL_NT = 640, 8192                         # Python integers at all positions up to these
U64 = (1 << 64) - 1
I64_MAX = (1 << 63) - 1
SHAPE_T = (2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 240, 241, 255, 256)
CHUNK = 64                                           # MPVSS_MAX_CHUNK of the `chunks` child
CHUNK_CASES = ((133, 7), (128, 64), (130, 65))       # (n, t)


class Modulus:
    def __init__(self, name, q, lpl, eb=256, safe=False):
        self.name, self.q, self.lpl, self.eb, self.safe = name, q, lpl, eb, safe
        self.bits = q.bit_length()
        self.top = (1 << (8 * eb)) - 1
        self.factor = None if safe else small_factor(q)

    @property
    def tiny(self):
        return self.q < 1 << 16


@functools.lru_cache(maxsize=None)
def _small_primes():
    sieve = bytearray([1]) * (1 << 16)
    for i in range(2, 256):
        if sieve[i]:
            sieve[i * i::i] = bytearray(len(sieve[i * i::i]))
    return [i for i in range(3, 1 << 16) if sieve[i]]


def small_factor(q):
    """the smallest prime factor of q below 2^16 that is not q itself, or None"""
    for p in _small_primes():
        if p * p > q:
            return None
        if q % p == 0:
            return p
    return None


def odd_modulus(bits):
    """H.random_odd_modulus of the first seed whose modulus has a prime factor below 2^16: a commitment that shares a factor with
    q needs one"""
    s = 0
    while True:
        q = H.random_odd_modulus(bits, random.Random(f"modp rt fd edges/{bits}/{s}"))
        if small_factor(q):
            return q
        s += 1


def all_ones_modulus(bits):
    """2^bits - c for the smallest c > 0 that makes it 3 mod 4 (not a prime: the identities need none): top limbs all ones"""
    c = 1
    while ((1 << bits) - c) % 4 != 3:
        c += 1
    return (1 << bits) - c


@functools.lru_cache(maxsize=None)
def moduli(width):
    sp = H.small_safe_primes()
    if width == "5":
        return (Modulus("q7", 7, 5, safe=True), Modulus("q23", 23, 5, safe=True), Modulus("p40", sp[40], 5, safe=True),
                Modulus("p64", sp[64], 5, safe=True), Modulus("p256", sp[256], 5, safe=True), Modulus("odd578", odd_modulus(578), 5))
    if width == "9":
        return (Modulus("odd579", odd_modulus(579), 9), Modulus("rfc1024", H.rfc_prime(1024), 9, safe=True),
                Modulus("odd1042", odd_modulus(1042), 9))
    if width == "18":
        return (Modulus("odd1043", odd_modulus(1043), 18), Modulus("rfc2048", H.rfc_prime(2048), 18, safe=True),
                Modulus("ones2048", all_ones_modulus(2048), 18))
    if width == "27":
        return (Modulus("odd2049", odd_modulus(2049), 27, WH.EB), Modulus("group15", WH.group15(), 27, WH.EB, safe=True),
                Modulus("ones3072", all_ones_modulus(3072), 27, WH.EB))
    raise KeyError(width)


def modulus(width, name):
    return next(m for m in moduli(width) if m.name == name)


# ---- the chain geometry (rt_commit_eval_dev, modp_rt_fd_chain, k_rt_fd_chain) -------------------------------------------------
def fd_chain(n, S, c):
    """mirror of modp_rt_fd_chain (modp_rt_kernels.h): chain c of S holds the run indices [first, first + len)"""
    a = c * n // S
    return a, (c + 1) * n // S - a


def fd_chains(n, t, chains):
    """S of rt_commit_eval_dev: the setting, or n / 4t (1 .. 32) when it is 0; at most n / t, so that every chain holds t positions"""
    S = chains if chains > 0 else max(1, min(32, n // (4 * t)))
    return max(1, min(S, n // t))


def fd_geometry(n, t, chains):
    """[(first, len, first seed)] of every chain: the seed rule first + (len - t) / 2"""
    S = fd_chains(n, t, chains)
    out = []
    for c in range(S):
        first, length = fd_chain(n, S, c)
        out.append((first, length, first + (length - t) // 2))
    return out


def sample_indices(n, t, chains, roots=()):
    """run indices for the Python integers where a case is too large for all of them"""
    if n < t:
        return sorted({0, n // 2, n - 1})
    s = set(roots)
    for first, length, seed0 in fd_geometry(n, t, chains):
        s |= {first, first + length - 1, seed0, seed0 + t - 1, seed0 - 1, seed0 + t}
    return sorted(i for i in s if 0 <= i < n)


def expected_path(q, given, p0, n, t_max):
    """the host gate in mode 2 (rt_fd_prepare, rt_fd_positions_ok, rt_commit_eval_dev) for n consecutive positions from p0.
    A negative position never reaches it: stage_positions refuses the call in either space (MPVSS_E_INVALID; the reference
    panics on a negative exponent) under every mode -- `invalid`"""
    t = len(given)
    if p0 < 0:
        return "invalid"
    if not 2 <= t <= t_max or n < t:
        return "horner"
    if any(math.gcd(c % q, q) != 1 for c in given):
        return "horner"
    if p0 + n - 1 > I64_MAX:
        return "horner"
    if q - 1 < 1 << 64 and p0 + n - 1 >= q - 1:
        return "horner"
    return "fd"


def ref_x(C, q, i):
    """X at position i as Python integers.  The position is what k_rt_commit_eval makes of the int64: its 64 bits as an unsigned
    number, reduced mod q - 1 when q - 1 is below 2^64.  Units: Horner's rule in the exponent (an integer identity);
    otherwise prod_j C_j^(i^j mod (q-1)), the reference's form"""
    i &= U64
    if q - 1 < 1 << 64:
        i %= q - 1
    C = [c % q for c in C]
    if all(math.gcd(c, q) == 1 for c in C):
        acc = C[-1]
        for c in reversed(C[:-1]):
            acc = pow(acc, i, q) * c % q
        return acc
    x = 1
    for j, c in enumerate(C):
        x = x * pow(c, pow(i, j, q - 1), q) % q
    return x


class Case:
    def __init__(self, cid, family, mod, given, p0, n, chains, space="host", roots=(), kind="x", t=None, path=None, note=""):
        self.id, self.family, self.mod, self.given, self.p0, self.n, self.chains, self.space = cid, family, mod, given, p0, n, chains, space
        self.kind, self.note = kind, note
        self.roots = list(roots)                         # run indices at which X = 1 is planted
        self.t = len(given) if given is not None else t
        self.q = mod.q
        self.path = path or expected_path(mod.q, given, p0, n, FD_MAX_T[mod.lpl])
        t = self.t
        if mod.bits <= ALL_BITS and n * t <= ALL_NT:
            self.at = list(range(n))
        else:
            self.at = sample_indices(n, t, chains, self.roots)

    @property
    def C(self):
        return [c % self.q for c in self.given]

    @property
    def positions(self):
        return list(range(self.p0, self.p0 + self.n))


def units(rng, q, k):
    out = []
    while len(out) < k:
        c = rng.randrange(2, q) if q > 3 else 2
        if math.gcd(c, q) == 1:
            out.append(c)
    return out


# ---- family A ----------------------------------------------------------------------------------------------------------------
def family_a(M, t, n, chains, p0):
    """the degenerate commitments of one modulus and shape"""
    q = M.q
    rng = random.Random(f"A/{M.name}/{t}/{n}")
    base = units(rng, q, t)
    mid = t // 2
    inv0 = pow(base[0], -1, q)
    sets = {
        "mid-one": base[:mid] + [1] + base[mid + 1:],
        "top-one": base[:-1] + [1],
        "constant": base[:1] + [1] * (t - 1),                 # X is constant: every D_k, k >= 1, is one
        "linear": [1] + base[1:2] + [1] * (t - 2),            # only C_1 is not one
        "all-one": [1] * t,
        "all-minus-one": [q - 1] * t,
        "mid-minus-one": base[:mid] + [q - 1] + base[mid + 1:],
        "all-equal": base[:1] * t,
        "alternating": [base[0] if j % 2 == 0 else inv0 for j in range(t)],
        "plus-kq": base[:1] + [base[1] + (M.top - base[1]) // q * q] + base[2:],      # the largest k that fits EB bytes
        "top-value": base[:1] + [M.top] + base[2:],           # 2^(8 EB) - 1: forward differences when it is a unit mod q
    }
    if M.factor:                                              # shares a factor with q, is not 0 mod q: Horner, the bytes of mode 0
        sets["non-unit"] = base[:1] + [M.factor] + base[2:]
        assert M.factor % q != 0 and (p0 + n) ** (t - 1) < q - 1       # i^j < q - 1: the reference's reduction changes nothing
    out = []
    for name, given in sets.items():
        assert len(given) == t and all(0 <= g <= M.top for g in given)
        out.append(Case(f"A-{M.name}-t{t}-p{p0}-{name}", "A", M, given, p0, n, chains))
    assert out[-1].path == "horner" or not M.factor
    return out


# ---- family B ----------------------------------------------------------------------------------------------------------------
def poly_mul(a, b, m):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % m
    return out


@functools.lru_cache(maxsize=None)
def _pow4_rows(q):
    """4^(d 16^i) mod q for every 4-bit window i of an exponent below q and every digit d"""
    rows, b = [], 4 % q
    for _ in range((q.bit_length() + 3) // 4):
        row = [1]
        for _ in range(15):
            row.append(row[-1] * b % q)
        rows.append(row)
        b = row[15] * b % q
    return rows


def pow4(a, q):
    """4^a mod q for 0 <= a < q through the fixed-base rows (family B takes some hundred powers of 4 per modulus)"""
    x, i, rows = 1, 0, _pow4_rows(q)
    while a:
        if a & 15:
            x = x * rows[i][a & 15] % q
        a >>= 4
        i += 1
    return x


def root_indices(n, t, chains, placement):
    """four run indices at which family B plants X = 1, through the mirror of the chain geometry.  Placement 1: the middle chain's
    first position, its last, its first seed and its last seed.  Placement 2: the positions next to that chain's seeds on both
    sides, the first position of the next chain, and the position after the seeds of the chain before"""
    g = fd_geometry(n, t, chains)
    assert len(g) >= 3
    first, length, seed0 = g[1]
    if placement == 1:
        idx = [first, first + length - 1, seed0, seed0 + t - 1]
    else:
        idx = [seed0 - 1, seed0 + t, g[2][0], g[0][2] + t]
    assert len(set(idx)) == 4 and all(0 <= i < n for i in idx)
    return idx


def family_b(M, t, placement):
    """C_j = 4^(a_j) with a(x) = b(x) prod (x - r_k) mod (q-1)/2, b of degree t - 5: X(r_k) = 1"""
    assert M.safe
    q, sub = M.q, (M.q - 1) // 2
    n, chains, p0 = 4 * t + 3, 3, (1 if placement == 1 else 1000)
    rng = random.Random(f"B/{M.name}/{t}/{placement}")
    idx = root_indices(n, t, chains, placement)
    a = [rng.randrange(sub) for _ in range(t - 5)] + [rng.randrange(1, sub)]
    for i in idx:
        a = poly_mul(a, [(-(p0 + i)) % sub, 1], sub)
    assert len(a) == t and pow4(a[-1], q) == pow(4, a[-1], q)
    return Case(f"B-{M.name}-t{t}-place{placement}", "B", M, [pow4(aj, q) for aj in a], p0, n, chains, roots=idx)


# ---- families C, D, E, F -----------------------------------------------------------------------------------------------------
def random_case(cid, family, M, t, p0, n, chains, space="host", seed=None):
    rng = random.Random(f"{family}/{M.name}/{t}/{seed if seed is not None else cid}")
    return Case(cid, family, M, units(rng, M.q, t), p0, n, chains, space)


def family_c(width):
    mods = [m for m in moduli(width) if not m.tiny]
    lpl = mods[0].lpl
    tmax = FD_MAX_T[lpl]
    ts = {"5": SHAPE_T, "9": (16, 17, 128, 129, 241, 256), "18": (16, 17, 128, 129, 241, 256), "27": (16, 17, 127, 128)}[width]
    out = []
    for k, t in enumerate(x for x in ts if x != tmax):        # t_max itself: below, on every modulus
        out.append(random_case(f"C-t{t}", "C", mods[k % len(mods)], t, (0, 1, 1000)[k % 3], 4 * t + 3, 3))
    t = 17
    shapes = (("no-steps", t, 3 * t, 3), ("one-direction", t, 3 * t + 1, 3), ("ragged", t, 3 * t + 2, 3), ("2t-1", t, 2 * t - 1, 1),
              ("long-chain", 3, 4099, 1), ("64-chains", 2, 4099, 64), ("clamped", t, 4099, 1000))
    for k, (name, tt, n, chains) in enumerate(shapes):
        out.append(random_case(f"C-{name}", "C", mods[(k + 1) % len(mods)], tt, 1, n, chains))
    for M in mods:                                            # the largest workgroup of the width
        out.append(random_case(f"C-tmax-{M.name}", "C", M, tmax, 1, 4 * tmax + 3, 3))
    out.append(random_case("C-tmax+1", "C", mods[-1], tmax + 1, 1, tmax + 10, 0))      # one past it: Horner's rule
    assert out[-1].path == "horner" and all(c.path == "fd" for c in out[:-1])
    return out


def family_d(width):
    M = modulus(width, {"5": "p256", "9": "rfc1024", "18": "rfc2048", "27": "group15"}[width])
    t, n = 5, 40
    out = []
    for label, p0 in (("0", 0), ("1", 1), ("2^32-20", (1 << 32) - 20), ("2^62", 1 << 62), ("2^63-n", (1 << 63) - n)):
        for space in ("host", "device"):
            out.append(random_case(f"D-{M.name}-p0={label}-{space}", "D", M, t, p0, n, 0, space, seed="D"))
            assert out[-1].path == "fd"
    if width == "5":
        M = modulus("5", "p64")                               # q - 1 has 64 bits: qm1_hi != 0, and Horner's % (q - 1) changes nothing
        assert (1 << 63) - 1 < M.q - 1 < 1 << 64
        for space in ("host", "device"):
            out.append(random_case(f"D-p64-p0=2^63-n-{space}", "D", M, t, (1 << 63) - n, n, 0, space, seed="D"))
            assert out[-1].path == "fd"
        for name, nn in (("q23", 20), ("p40", n)):
            M = modulus("5", name)
            q = M.q
            for label, p0, path in (("ends-q-2", q - 1 - nn, "fd"), ("ends-q-1", q - nn, "horner")):
                out.append(random_case(f"D-{name}-{label}", "D", M, t, p0, nn, 0, seed="D"))
                assert out[-1].path == path
            for space in ("host", "device"):     # refused before any launch decision, whatever the mode
                out.append(random_case(f"D-{name}-p0=-5-{space}", "D", M, t, -5, nn, 0, space, seed="D"))
                assert out[-1].path == "invalid"
    return out


def family_e(width):
    """state kept in the context between calls (rt_cm_inv, rt_fd_seeds, rt_fd_park, rt_fd_ready): the order is the point"""
    if width == "18":
        A, B, Z = modulus("18", "rfc2048"), modulus("18", "odd1043"), modulus("5", "p256")
    elif width == "27":
        A, B, Z = modulus("27", "group15"), modulus("27", "odd2049"), None
    else:
        return []
    tmax = FD_MAX_T[A.lpl]
    rng = random.Random(f"E/{width}")
    shared = []                                               # the same t = 5 commitments for every handle
    while len(shared) < 5:
        c = rng.randrange(2, 1 << 200)
        if all(math.gcd(c, m.q) == 1 for m in (A, B, Z) if m):
            shared.append(c)
    bad = shared[:2] + [B.factor] + shared[3:]
    out = [random_case("E-1-tmax", "E", A, tmax, 1, 4 * tmax + 3, 3)]
    if Z:
        out.append(random_case("E-1z-narrow-t33", "E", Z, 33, 1, 135, 3))
    out.append(random_case("E-2-t2-same-handle", "E", A, 2, 1, 11, 2))
    out.append(Case("E-3a-t5-handle-a", "E", A, shared, 7, 23, 3))
    out.append(Case("E-3b-t5-handle-b", "E", B, shared, 7, 23, 3))
    if Z:
        out.append(Case("E-3z-t5-narrow", "E", Z, shared, 7, 23, 3))
    out.append(Case("E-4-non-unit", "E", B, bad, 7, 23, 3))
    out.append(Case("E-5-admissible-same-t", "E", B, shared, 7, 23, 3))
    if Z:
        out.append(random_case("E-5z-narrow-t2", "E", Z, 2, 0, 9, 1))
    out.append(Case("E-6-non-unit-again", "E", B, bad, 7, 23, 3))
    out.append(Case("E-7a-device", "E", A, shared, 7, 23, 3, "device"))
    out.append(Case("E-7b-host", "E", A, shared, 7, 23, 3, "host"))
    assert [c.path for c in out if c.id.startswith(("E-4", "E-6"))] == ["horner", "horner"]
    assert all(c.path == "fd" for c in out if not c.id.startswith(("E-4", "E-6")))
    return out


BOX_N, BOX_T, BOX_ZERO = 40, 9, (2, 5, 8)


def family_f(width):
    """a whole box whose secret polynomial has zero coefficients: group_verify_distribution (honest and with one tampered share) and
    group_distribute under both modes"""
    name = {"5": "p256", "18": "rfc2048"}.get(width)
    if not name:
        return []
    M = modulus(width, name)
    return [Case(f"F-{name}-{what}", "F", M, None, 1, BOX_N, 0, kind=what, t=BOX_T, path="fd") for what in ("verify", "tampered", "distribute")]


def box_instance(q, n, t, zero, seed):
    """a box of the oracle's own dealer over the group of q whose coefficients a_j, j in `zero`, are 0 (their commitments are 1)"""
    import mpvss_oracle as O
    g = H.RtOracleGroup(q)
    rng = random.Random(seed)
    pks, seen = [], set()
    while len(pks) < n:
        pk = g.generate_public_key(H.keygen(g, rng))
        if pk not in seen:
            seen.add(pk)
            pks.append(pk)
    coeffs = [0 if j in zero else rng.randrange(1, g.q - 1) for j in range(t)]
    ws = [H.keygen(g, rng) for _ in range(n)]
    return g, pks, coeffs, ws, O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)


@functools.lru_cache(maxsize=None)
def build_cases(width):
    """every case of one width, in the order the child runs them"""
    cases = []
    for M in moduli(width):
        if M.name == "q7":            # q - 1 = 6: runs of 5 positions from 0, of 4 from 1
            shapes = [(2, 5, 0), (5, 5, 0), (2, 4, 1), (4, 4, 1)]
        elif M.name == "q23":         # q - 1 = 22
            shapes = [(2, 21, 0), (5, 21, 0), (21, 21, 0), (2, 20, 1), (5, 20, 1)]
        else:
            shapes = [(5, 23, 1), (33, 135, 1)]
        for t, n, p0 in shapes:
            cases += family_a(M, t, n, 3, p0)
    for M in moduli(width):
        if M.safe and not M.tiny and M.name != "p64":
            cases += [family_b(M, t, placement) for t in (9, 37) for placement in (1, 2)]
    cases += family_c(width) + family_d(width) + family_f(width) + family_e(width)
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


def expected(width):
    """case id -> the path its line must report"""
    if width == "chunks":
        return {f"chunks-n{n}-t{t}-{what}": path for (n, t), paths in zip(CHUNK_CASES, CHUNK_PATHS) for what, path in paths.items()}
    return {c.id: c.path for c in build_cases(width)}


# What a call of MPVSS_MAX_CHUNK = 64 counts in mpvss_modp_group_fd_stats under mode 2, as `fd=<chunks>,horner=<chunks>`.
# group_commit_eval is one pass whatever its size, but rt_fd_prepare judges t against min(n, MAX_CHUNK); group_verify_distribution
# runs chunks of 64.  (133, 7): 64, 64 and 5 -- the last chunk is below t.  (128, 64): two chunks of cnt == t, seeds only.
# (130, 65): t is above the chunk, the whole call takes Horner.
CHUNK_PATHS = (
    {"commit_eval": "fd=1,horner=0", "verify": "fd=2,horner=1"},
    {"commit_eval": "fd=1,horner=0", "verify": "fd=2,horner=0"},
    {"commit_eval": "fd=0,horner=1", "verify": "fd=0,horner=3"},
)


# ---- the GPU side ------------------------------------------------------------------------------------------------------------
class Mismatch(Exception):
    pass


def cat(vals, eb):
    return b"".join(v.to_bytes(eb, "big") for v in vals)


def split(b, eb):
    return [int.from_bytes(b[i:i + eb], "big") for i in range(0, len(b), eb)]


class Runner:
    def __init__(self):
        import torch
        from mpvss_rs_amd import Engine, capi
        self.torch, self.capi = torch, capi
        self.eng = Engine(0)
        self.groups = {}
        self.boxes = {}

    def group(self, M):
        from mpvss_rs_amd import ModpGroup
        if M.name not in self.groups:
            grp = ModpGroup(M.q, elem_bytes=M.eb) if M.eb != 256 else ModpGroup(M.q)
            assert (grp.elem_bytes, grp.limbs_per_lane, grp.fd_max_t) == (M.eb, M.lpl, FD_MAX_T[M.lpl]), M.name
            self.groups[M.name] = grp
        return self.groups[M.name]

    def commit_eval(self, grp, cb, positions, space):
        eng, torch = self.eng, self.torch
        if space == "host":
            return eng.group_commit_eval(grp, cb, positions)
        eb, n = grp.elem_bytes, len(positions)
        d_c = torch.frombuffer(bytearray(cb), dtype=torch.uint8).cuda()
        d_p = torch.tensor(positions, dtype=torch.int64).cuda()
        d_o = torch.zeros(n * eb, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()          # torch's copies run on torch's stream, the engine's kernels on the engine's
        eng.group_commit_eval_device(grp, d_c.data_ptr(), len(cb) // eb, d_p.data_ptr(), n, d_o.data_ptr())
        return bytes(d_o.cpu().numpy())

    def both_modes(self, call, chains):
        """call() under mode 2 and under mode 0: (result of mode 2, (fd, horner) chunks it counted, result of mode 0)"""
        eng = self.eng
        eng.set_rt_fd(2, chains)
        s0 = eng.group_fd_stats()
        got = call()
        s1 = eng.group_fd_stats()
        eng.set_rt_fd(0, 0)
        ref = call()
        s2 = eng.group_fd_stats()
        eng.set_rt_fd(2, 0)
        if not (s2["fd"] == s1["fd"] and s2["horner"] > s1["horner"]):
            raise Mismatch(f"mode 0 did not take Horner's rule: {s1} -> {s2}")
        return got, (s1["fd"] - s0["fd"], s1["horner"] - s0["horner"]), ref

    @staticmethod
    def path_of(delta):
        if (delta[0] > 0) == (delta[1] > 0):
            raise Mismatch(f"fd_stats moved by {delta}: not one path")
        return "fd" if delta[0] > 0 else "horner"

    def run_invalid(self, case, grp, cb):
        """a call the entry point refuses: MPVSS_E_INVALID under both modes, and neither path is counted"""
        from mpvss_rs_amd import EngineError
        eng = self.eng
        for mode in (2, 0):
            eng.set_rt_fd(mode, case.chains if mode else 0)
            s0 = eng.group_fd_stats()
            try:
                self.commit_eval(grp, cb, case.positions, case.space)
            except EngineError as e:
                if "rc=-1" not in str(e) or "negative position" not in str(e):
                    raise Mismatch(f"mode {mode}: refused, but not as a negative position: {e}")
            else:
                raise Mismatch(f"mode {mode}: a negative position was accepted")
            if eng.group_fd_stats() != s0:
                raise Mismatch(f"mode {mode}: a refused call was counted")
        eng.set_rt_fd(2, 0)
        return b"", "invalid"

    def run_x(self, case):
        grp = self.group(case.mod)
        eb, q = grp.elem_bytes, case.q
        cb = cat(case.given, eb)
        positions = case.positions
        if case.path == "invalid":
            return self.run_invalid(case, grp, cb)
        got, delta, ref = self.both_modes(lambda: self.commit_eval(grp, cb, positions, case.space), case.chains)
        path = self.path_of(delta)
        if path != case.path:
            raise Mismatch(f"took {path}, expected {case.path}")
        if len(got) != case.n * eb or got != ref:
            bad = [i for i in range(case.n) if got[i * eb:(i + 1) * eb] != ref[i * eb:(i + 1) * eb]]
            raise Mismatch(f"{len(bad)} of {case.n} X differ between mode 2 and mode 0, first at run indices {bad[:12]} "
                           f"(chains {fd_geometry(case.n, case.t, case.chains) if case.n >= case.t else None})")
        vals = split(got, eb)
        C = case.C
        for i in case.at:
            want = ref_x(C, q, positions[i])
            if vals[i] != want:
                raise Mismatch(f"X at run index {i} (position {positions[i]}) is not what Python integers give (both modes agree)")
        for i in case.roots:
            if vals[i] != 1:
                raise Mismatch(f"X at the planted root, run index {i}, is not 1")
        return got, path

    def box(self, M):
        if M.name not in self.boxes:
            import mpvss_oracle as O
            g, pks, coeffs, ws, box = box_instance(M.q, BOX_N, BOX_T, BOX_ZERO, f"F/{M.name}")
            assert all(box["commitments"][j] == 1 for j in BOX_ZERO)
            keys = [g.element_to_bytes(p) for p in pks]
            positions = list(range(1, BOX_N + 1))
            self.boxes[M.name] = dict(g=g, pks=pks, ws=ws, box=box, positions=positions, Y=[box["shares"][k] for k in keys],
                                      R=[box["responses"][k] for k in keys],
                                      P=[O.poly_get_value(coeffs, i) % (g.q - 1) for i in positions])
        return self.boxes[M.name]

    def run_box(self, case):
        eng, grp, k = self.eng, self.group(case.mod), self.box(case.mod)
        eb, box = grp.elem_bytes, k["box"]
        Cm, pk, ch = cat(box["commitments"], eb), cat(k["pks"], eb), cat([box["challenge"]], eb)
        Y, R = cat(k["Y"], eb), cat(k["R"], eb)
        if case.kind == "distribute":
            d, delta, d0 = self.both_modes(lambda: eng.group_distribute(grp, Cm, k["positions"], pk, cat(k["P"], eb), cat(k["ws"], eb)), 0)
            if d != d0:
                raise Mismatch("group_distribute differs between mode 2 and mode 0")
            if split(d["X"], eb) != box["_X"] or d["digest"] != box["_digest"] or split(d["Y"], eb) != k["Y"]:
                raise Mismatch("group_distribute: X, Y or the digest are not the oracle's")
            return d["X"] + d["digest"], self.path_of(delta)
        if case.kind == "tampered":
            bad = bytearray(Y)
            bad[7 * eb + eb - 1] ^= 1
            Y = bytes(bad)
        v, delta, v0 = self.both_modes(lambda: eng.group_verify_distribution(grp, Cm, k["positions"], pk, Y, R, ch, dump=True), 0)
        if v != v0:
            raise Mismatch("group_verify_distribution differs between mode 2 and mode 0")
        if split(v["X"], eb) != box["_X"]:
            raise Mismatch("group_verify_distribution: X is not the oracle's")
        if case.kind == "verify" and not (v["verdict"] is True and v["digest"] == box["_digest"]):
            raise Mismatch("the verifier rejects the dealer's own box, or its digest is not the oracle's")
        if case.kind == "tampered" and not (v["verdict"] is False and v0["verdict"] is False):
            raise Mismatch("a tampered share is accepted")
        return v["X"] + v["digest"] + bytes([v["verdict"]]), self.path_of(delta)

    def run_chunks(self):
        import mpvss_oracle as O
        eng = self.eng
        assert os.environ.get("MPVSS_MAX_CHUNK") == str(CHUNK), "the chunks child runs with MPVSS_MAX_CHUNK=64"
        M = modulus("5", "p256")
        grp = self.group(M)
        eb, q = grp.elem_bytes, M.q
        for (n, t), paths in zip(CHUNK_CASES, CHUNK_PATHS):
            g, pks, coeffs, ws, box = box_instance(q, n, t, (), f"chunks/{n}/{t}")
            keys = [g.element_to_bytes(p) for p in pks]
            positions = list(range(1, n + 1))
            Cm, pk, ch = cat(box["commitments"], eb), cat(pks, eb), cat([box["challenge"]], eb)
            Y, R = cat([box["shares"][k] for k in keys], eb), cat([box["responses"][k] for k in keys], eb)
            want = [ref_x(box["commitments"], q, i) for i in positions]
            assert want == box["_X"]
            for what, call in (("commit_eval", lambda: eng.group_commit_eval(grp, Cm, positions)),
                               ("verify", lambda: eng.group_verify_distribution(grp, Cm, positions, pk, Y, R, ch, dump=True))):
                cid = f"chunks-n{n}-t{t}-{what}"
                try:
                    got, delta, ref = self.both_modes(call, 0)
                    path = f"fd={delta[0]},horner={delta[1]}"
                    if path != paths[what]:
                        raise Mismatch(f"fd_stats advanced by {delta}, expected {paths[what]}")
                    if got != ref:
                        raise Mismatch("mode 2 and mode 0 differ")
                    x = got if what == "commit_eval" else got["X"]
                    if split(x, eb) != want:
                        raise Mismatch("X is not what Python integers give")
                    if what == "verify" and not (got["verdict"] is True and got["digest"] == box["_digest"]):
                        raise Mismatch("verdict or digest are not the oracle's")
                except Exception as e:
                    fail(cid, e)
                print("case", cid, hashlib.sha256(x).hexdigest(), path, flush=True)


def fail(cid, e):
    print(f"MISMATCH in case {cid}: {type(e).__name__}: {e}", flush=True)
    sys.exit(1)


def run(width):
    r = Runner()
    if width == "chunks":
        r.run_chunks()
    else:
        for case in build_cases(width):
            try:
                got, path = r.run_x(case) if case.kind == "x" else r.run_box(case)
            except Exception as e:        # a refused launch (EngineError) names its case too
                fail(case.id, e)
            print("case", case.id, hashlib.sha256(got).hexdigest(), path, flush=True)
    r.eng.close()
    print(f"modp rt fd edges {width} ok", flush=True)


if __name__ == "__main__":
    import torch  # noqa: F401  (torch's HIP runtime first, as tests/conftest.py)
    run(sys.argv[1])
