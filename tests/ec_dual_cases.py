"""Cases for the curve groups' windowed double-scalar kernel (dual_win_body / dual_win_glv_body in csrc/ec_kernels.hip):
scalars at the edges of the signed 4-bit recoding and of secp256k1's endomorphism split, bases at the edges of the group
law, and a pool of all-distinct rows for the lane and workgroup edges.  Needs neither torch nor a GPU:
tests/test_ec_dual_cases.py holds the cases to their claims on the CPU, tests/test_gpu_ec_dual_edges.py sends them through
the engine.

A row is (tag, g1, h1, g2, h2, r, c): four encodings and two reduced scalars (integers); the kernels compute
a1 = r g1 + c h1 and a2 = r g2 + c h2.  mpvss_ec_dleq_commitments takes ONE g1 per call, so a call uses the group
generator (`Cases.gen`, the comb) or the curve's shared non-generator point (`Cases.p0`, a second table) whatever the
row holds; the rows of the grids carry p0 there, the rows of the pools a point of their own that serves as the base
of the one-scalar calls.

Expected values come from oracle/ec_ref.c (plain double-and-add, no windows, no endomorphism), computed once per
process and cached."""
import ctypes as C
import functools
import os
import random
import re
import subprocess
from collections import namedtuple

import mpvss_oracle as O
from ec_ref import GROUP_ID, EcRef

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("secp256k1", "ristretto255")
Row = namedtuple("Row", "tag g1 h1 g2 h2 r c")

# lane and workgroup edges of a 256-lane workgroup of 64-lane waves; 513: a third workgroup with one live lane
SHAPES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)
EXTRACT_SHAPES = (1, 64, 257, 513)
POOL = 331                      # prime and above 256: lanes 1, 64 or 256 apart never hold the same pool row
LANE_DISTANCES = (1, 64, 256)

# (sign k1, sign k2, top digit k1, top digit k2) of k = k1 + k2 lambda: what 4000 seeded draws fall into
CLASS_SEED, CLASS_DRAWS = 0xD0A1, 4000
GLV_CLASSES = frozenset({(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0),
                         (0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 1), (1, 1, 1, 0)})

EXTREME_WINDOWS = (0, 7, 8, 31, 32, 63)     # first / last nibble of a word of the recoded scalar, of the low half, the top one
HALF_WINDOWS = (0, 7, 8, 31)                # the same for a 128-bit half of secp256k1's split (its window 32 is the top digit)
DIGIT_GRID_MAX = 800                        # rows of EDGE x EDGE kept: beyond it a Latin-square selection (digit_pairs)


# ---- the host shim (the kernels' own scalar code compiled for the CPU) ---------------------------------------------
def load_shim():
    """tests/ec_host_shim.cpp as a shared library (built as tests/test_ec_host.py builds it)"""
    lib = os.path.join(HERE, "_build", "libec_host.so")
    src = os.path.join(HERE, "ec_host_shim.cpp")
    deps = [src, os.path.join(HERE, "ec_repr_ops.h")] + \
        [os.path.join(HERE, "..", "mpvss_rs_amd", "csrc", f)
         for f in ("ec_field.h", "ec_curves.h", "ec_consts.h", "ec_glv.h", "ec_scalar.h", "ec_keyset.h")]
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        tmp = "%s.%d" % (lib, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", tmp])
        os.replace(tmp, lib)
    return C.CDLL(lib)


@functools.lru_cache(maxsize=None)
def _shim():
    return load_shim()


def glv_lambda():
    """lambda of secp256k1's endomorphism, read from tools/gen_ec_consts.py (importing that tool would rewrite ec_consts.h)"""
    text = open(os.path.join(HERE, "..", "tools", "gen_ec_consts.py")).read()
    lam = int(re.search(r"^GLV_LAMBDA = (0x[0-9a-fA-F]+)", text, re.M).group(1), 16)
    assert pow(lam, 3, O.SECP_N) == 1 and lam != 1
    return lam


def glv_split(k):
    """(|k1|, sign k1, |k2|, sign k2) of a secp256k1 scalar as ec_glv.h splits it"""
    out = (C.c_uint8 * 36)()
    assert _shim().secp_glv_split_bytes((C.c_uint8 * 32).from_buffer_copy(k.to_bytes(32, "big")), out) == 0
    raw = bytes(out)
    return int.from_bytes(raw[0:17], "little"), raw[17], int.from_bytes(raw[18:35], "little"), raw[35]


# ---- the recoding model -----------------------------------------------------------------------------------------------
def recoded_nibbles(k, windows=64):
    """nibbles 0 .. windows-1 of k + 0x88..8 and the carry as nibble `windows`: digit w is nibble w minus 8 below the
    top, the top nibble itself there (ec_kernels.hip, signed 4-bit Straus)"""
    K = k + int("8" * windows, 16)
    return [(K >> (4 * w)) & 15 for w in range(windows)] + [K >> (4 * windows)]


def glv_class(k):
    m1, s1, m2, s2 = glv_split(k)
    return (s1, s2, recoded_nibbles(m1, 32)[32], recoded_nibbles(m2, 32)[32])


def glv_class_search(order):
    """[(class, first scalar of that class)] in the order of first occurrence among the seeded draws"""
    rng = random.Random(CLASS_SEED)
    seen = {}
    for _ in range(CLASS_DRAWS):
        k = rng.randrange(order)
        seen.setdefault(glv_class(k), k)
    return list(seen.items())


def _with_nibble(K, w, nib):
    return (K & ~(15 << (4 * w))) | (nib << (4 * w))


def full_extreme(rng, order, w, nib):
    """a reduced scalar whose recoded nibble w is `nib` (0: digit -8, the table entry 8P; 15: digit +7), or None when
    no reduced scalar has it"""
    off = int("8" * 64, 16)
    for _ in range(200):
        k = _with_nibble(rng.randrange(order) + off, w, nib) - off
        if 0 <= k < order and recoded_nibbles(k)[w] == nib:
            return k
    return None


def half_extreme(rng, order, lam, w, nibs):
    """a reduced secp256k1 scalar whose halves k1, k2 have the recoded nibbles nibs[0], nibs[1] at window w (as the
    shim splits it)"""
    off = int("8" * 32, 16)
    for _ in range(4000):
        ms = [_with_nibble(rng.getrandbits(128) + off, w, nibs[j]) - off for j in range(2)]
        if min(ms) < 0:
            continue
        k = (rng.choice((1, -1)) * ms[0] + rng.choice((1, -1)) * ms[1] * lam) % order
        m1, _, m2, _ = glv_split(k)
        if recoded_nibbles(m1, 32)[w] == nibs[0] and recoded_nibbles(m2, 32)[w] == nibs[1]:
            return k
    raise AssertionError("no scalar with half nibbles %r at window %d" % (nibs, w))


def digit_pairs(m, limit=DIGIT_GRID_MAX):
    """index pairs (i, j) of the digit grid: all m * m when they fit, else the Latin-square selection
    j = i + s (mod m) for as many shifts s as fit, spread evenly over 0 .. m - 1 (0 among them: every value meets itself)
    -- every value still appears as r and as c, equally often"""
    if m * m <= limit:
        return [(i, j) for i in range(m) for j in range(m)]
    count = max(1, limit // m)
    shifts = [(j * m) // count for j in range(count)]
    return [(i, (i + s) % m) for s in shifts for i in range(m)]


# ---- the cases of one curve ----------------------------------------------------------------------------------------------
class Cases:
    def __init__(self, name):
        self.name = name
        self.G = G = O.GROUPS[name]()
        self.gid = GROUP_ID[name]
        self.order = order = G.group_order_int()
        self.L = G.elem_len
        self.ref = EcRef()
        self.gen = G.element_to_bytes(G.generator())
        self.ident = bytes(self.L)
        self._dual, self._exp = {}, {}        # the reference's results: rows, single multiplications
        assert self.ident == G.element_to_bytes(G.identity())
        self.rng = rng = random.Random(0xEC0D + self.gid)
        self.p0 = self.point()
        self.rand_r, self.rand_c = rng.randrange(1, order), rng.randrange(1, order)
        secp = name == "secp256k1"

        # -- scalars: (tag, value); EDGE's head is the `special` list of tests/test_gpu_ec.py
        special = [0, 1, 2, 7, 8, 9, 15, 16, 0x88888888, 0x77777777, (0x8 << 252) % order, order - 1, order - 2,
                   int("8" * 62, 16), int("7" * 63, 16) % order, int("f" * 63, 16) % order]
        edge = [("special %d" % i, k) for i, k in enumerate(special)]
        self.classes = []                     # [(class, scalar)]
        self.extremes = []                    # [(scalar, scope, window, nibble)]: scope "full", or "halves" with a nibble pair
        self.unreachable = []                 # [(window, nibble)] no reduced scalar of this curve has
        if secp:
            self.lam = lam = glv_lambda()
            edge += [("lambda", lam), ("n - lambda", order - lam), ("lambda + 1", lam + 1), ("lambda - 1", lam - 1),
                     ("lambda^2", lam * lam % order), ("2^128 - 1", (1 << 128) - 1), ("2^128", 1 << 128), ("2^127", 1 << 127)]
            self.classes = glv_class_search(order)
            edge += [("class %r" % (cl,), k) for cl, k in self.classes]
        for nib in (0, 15):
            for w in EXTREME_WINDOWS:
                k = full_extreme(rng, order, w, nib)
                if k is None:
                    self.unreachable.append((w, nib))
                    continue
                self.extremes.append((k, "full", w, nib))
                edge.append(("nibble %d at window %d" % (nib, w), k))
        if secp:
            k = rng.randrange(int("7" * 63 + "8", 16), order)      # the comb's 65th digit is 1
            self.extremes.append((k, "full", 64, 1))
            edge.append(("65th digit 1", k))
            for w in HALF_WINDOWS:
                for nibs in ((0, 15), (15, 0)):
                    k = half_extreme(rng, order, lam, w, nibs)
                    self.extremes.append((k, "halves", w, nibs))
                    edge.append(("half nibbles %r at window %d" % (nibs, w), k))
        self.edge = edge

        # -- grids
        self.digit_grid = []
        for i, j in digit_pairs(len(edge)):
            P, Q = self.point(), self.point()
            self.digit_grid.append(Row("r: %s / c: %s" % (edge[i][0], edge[j][0]), self.p0, P, Q, P, edge[i][1], edge[j][1]))
        self.class_grid = []
        for ca, ka in self.classes:
            for cb, kb in self.classes:
                P, Q = self.point(), self.point()
                self.class_grid.append(Row("r: class %r / c: class %r" % (ca, cb), self.p0, P, Q, P, ka, kb))
        self.base_scalars = [(0, 0), (1, order - 1), (order - 1, order - 1), (0, self.rand_c), (self.rand_r, 0), (8, order - 8),
                             (self.rand_r, self.rand_c)]
        self.base_grid = []
        for tag, (h1, g2, h2) in self.base_triples():
            for r, c in self.base_scalars:
                self.base_grid.append(Row("bases %s, r = %#x, c = %#x" % (tag, r, c), self.p0, h1, g2, h2, r, c))

        # -- lane pools: all-distinct rows, and rows that share ONE challenge
        self.pool = [Row("pool row %d" % i, self.point(), self.point(), self.point(), self.point(), rng.randrange(1, order),
                         rng.randrange(1, order)) for i in range(POOL)]
        shared_c = rng.randrange(1, order)
        self.pool_shared = [Row("shared-challenge pool row %d" % i, self.point(), self.point(), self.point(), self.point(),
                                rng.randrange(1, order), shared_c) for i in range(POOL)]

    # -- points
    def scalar(self, k):
        return self.G.scalar_to_fixed(k)

    def mul(self, point, k):
        """k * point by the plain-C reference, cached"""
        key = (point, k)
        if key not in self._exp:
            self._exp[key] = self.ref.exp(self.gid, point, self.scalar(k % self.order))
        return self._exp[key]

    def point(self):
        """a random point that is neither the identity nor the generator"""
        return self.mul(self.gen, self.rng.randrange(2, self.order))

    def neg(self, point):
        return self.mul(point, self.order - 1)

    def base_triples(self):
        """[(tag, (h1, g2, h2))]"""
        I, Gn = self.ident, self.gen
        out = []
        for tag in ("P Q P", "I Q P", "P I Q", "P Q I", "P P P", "P P -P", "G G -G", "I I I", "P G Q") + \
                (("P P phi(P)",) if self.name == "secp256k1" else ()):
            P, Q = self.point(), self.point()
            sym = {"P": P, "Q": Q, "I": I, "G": Gn}
            sym["-P"], sym["-G"] = self.neg(P), self.neg(Gn)
            if self.name == "secp256k1":
                sym["phi(P)"] = self.mul(P, self.lam)
            out.append((tag, tuple(sym[s] for s in tag.split())))
        return out

    # -- shapes
    def lane_rows(self, n, shared=False):
        """the rows of a launch of n shares: lane i holds pool row (i + n) mod 331"""
        pool = self.pool_shared if shared else self.pool
        return [pool[(i + n) % POOL] for i in range(n)]

    # -- expected values
    def expected(self, row, path):
        """(a1, a2) of a row with g1 = the generator (path "G") or the shared point p0 (path "P")"""
        key = (row.h1, row.g2, row.h2, row.r, row.c)
        if key not in self._dual:
            r, c = self.scalar(row.r), self.scalar(row.c)
            _, a1, a2 = self.ref.share_work(self.gid, row.h1, 1, row.g2, row.h2, r, c)       # a1 = r G + c h1, a2 = r g2 + c h2
            self._dual[key] = (a1, a2)
        a1, a2 = self._dual[key]
        if path == "P":
            key = ("P", row.h1, row.r, row.c)
            if key not in self._dual:
                self._dual[key] = self.ref.share_work(self.gid, row.h1, 1, self.p0, row.h1, self.scalar(row.r),
                                                      self.scalar(row.c))[2]               # r p0 + c h1
            a1 = self._dual[key]
        return a1, a2

    def grids(self):
        return [("digit grid", self.digit_grid), ("class grid", self.class_grid), ("base grid", self.base_grid)]


@functools.lru_cache(maxsize=None)
def cases(name):
    return Cases(name)


def cat(rows, field):
    return b"".join(getattr(r, field) for r in rows)


def scalars(cs, rows, field):
    return b"".join(cs.scalar(getattr(r, field)) for r in rows)
