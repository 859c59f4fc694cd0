"""Representatives for the curve kernels' lazily reduced field (mpvss_rs_amd/csrc/ec_field.h: 10 limbs of 26 bits, a limb
vector v stands for sum v[i] 2^(26 i) mod p) and points written with them.  Needs neither torch nor a GPU.

Any limb vector is a representative of some field element, so the reference value of a vector is always the Python integer
`value(v) % p`, never something the code under test says.  The classes below are the limb bounds ec_field.h states for
what its operations hand on; a stored coordinate may be in any of them, so the point cases use their union U.

A point case is P = a G, Q = b G for fixed seeded scalars.  One coordinate of each point is FREE: the whole projective /
extended point is scaled by lambda so that this coordinate is the value of a chosen free vector (saturated limbs in every
position); the other coordinates get representatives derived from their forced values.  Expected encodings come from
oracle/ec_ref.c through ec_dual_cases.Cases, which caches them.
tests/test_ec_repr_cases.py holds the module to its claims; tests/test_ec_repr_host.py (CPU), tests/test_gpu_ec_repr.py and
tests/test_gpu_ec_quad_repr.py (GPU) feed the cases to the code."""
import functools
import os
import random
import re
import struct
from collections import namedtuple

import mpvss_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("secp256k1", "ristretto255")
PRIMES = {"secp256k1": O.SECP_P, "ristretto255": O.ED_P}
PRIME_STRUCT = {"secp256k1": "PrimeSecp", "ristretto255": "PrimeEd"}
COORDS = {"secp256k1": "XYZ", "ristretto255": "XYZT"}          # the order of the words of a Point
NLIMB, LIMB_BITS = 10, 26

# ---- limb classes: (exclusive bound per limb, the line of ec_field.h it is taken from) -----------------------------------
CLASSES = {
    "carried": ([2**26 + 2**21, 2**27] + [2**26] * 8,
                "carry: 'out: v[0] < 2^26 + 2^21, v[1] < 2^27, others < 2^26'"),
    "product": ([2**26, 2**27] + [2**27 + 2**12] * 8,
                "reduce_columns: 'Out: v[0] < 2^26, v[1] < 2^27, v[2..9] < 2^27 + 2^12'"),
    "mul_small": ([2**27, 2**26 + 2**22] + [2**26] * 8,
                  "mul_small: 'out: v[0] < 2^27, v[1] < 2^26 + 2^22, others < 2^26'"),
    "U": ([2**27 + 2**12] * 10, "the union of the three: what a stored coordinate may be"),
    # not a class of stored coordinates: what mul / sqr accept, the home of the subtraction pad as a vector
    "mul input": ([2**30] * 10, "header: 'mul accepts limbs up to 2^30'"),
}
U = CLASSES["U"][0]
KINDS = ("canonical", "canonical + p", "top-heavy", "bottom-heavy")


def value(v):
    return sum(int(x) << (LIMB_BITS * i) for i, x in enumerate(v))


def limbs(x):
    """the canonical limbs of 0 <= x < 2^260"""
    assert 0 <= x < 1 << (LIMB_BITS * NLIMB)
    return [(x >> (LIMB_BITS * i)) & (2**LIMB_BITS - 1) for i in range(NLIMB)]


def in_class(v, bounds):
    return len(v) == NLIMB and all(0 <= x < b for x, b in zip(v, bounds))


def header_table(name, table):
    """the ten words of PrimeConsts<prime>::p or ::subpad, read from ec_consts.h"""
    text = open(os.path.join(HERE, "..", "mpvss_rs_amd", "csrc", "ec_consts.h")).read()
    block = text[text.index("struct PrimeConsts<%s>" % PRIME_STRUCT[name]):]
    m = re.search(r"u32 %s\(int i\) \{ constexpr u32 t\[10\] = \{([^}]*)\}" % table, block)
    return [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")]


def top_heavy(val, p, bounds):
    """val plus the largest multiple of p that fits the class, limbs filled from the top, each as large as it can be"""
    most = sum((b - 1) << (LIMB_BITS * i) for i, b in enumerate(bounds))
    rem = val + (most - val) // p * p
    out = [0] * NLIMB
    for i in range(NLIMB - 1, -1, -1):
        out[i] = min(bounds[i] - 1, rem >> (LIMB_BITS * i))
        rem -= out[i] << (LIMB_BITS * i)
    assert rem == 0
    return out


def bottom_heavy(val, bounds):
    """the canonical form with one unit of every limb moved into 2^26 of the limb below, while that fits"""
    out = limbs(val)
    for i in range(NLIMB - 1, 0, -1):
        while out[i] >= 1 and out[i - 1] + 2**LIMB_BITS < bounds[i - 1]:
            out[i] -= 1
            out[i - 1] += 2**LIMB_BITS
    return out


def representatives(val, p, bounds, free=False):
    """[(kind, vector)] of val mod p in the class `bounds`; with free=True the free vectors too, which stand for whatever
    value they happen to have"""
    val %= p
    plus_p = [a + b for a, b in zip(limbs(val), limbs(p))]             # uncarried
    out = [("canonical", limbs(val)), ("canonical + p", plus_p), ("top-heavy", top_heavy(val, p, bounds)),
           ("bottom-heavy", bottom_heavy(val, bounds))]
    out = [(k, v) for k, v in out if in_class(v, bounds)]
    return out + (free_vectors(bounds) if free else [])


def free_vectors(bounds):
    top = [b - 1 for b in bounds]
    out = [("all limbs at the bound", top),
           ("even limbs at the bound", [t if i % 2 == 0 else 0 for i, t in enumerate(top)]),
           ("odd limbs at the bound", [t if i % 2 == 1 else 0 for i, t in enumerate(top)])]
    return out + [("limb %d at the bound" % k, [t if i == k else 0 for i, t in enumerate(top)]) for k in range(NLIMB)]


def zero_representatives(name):
    """[(tag, vector, class)]: limb vectors that are = 0 mod p without being 0"""
    p = PRIMES[name]
    pl = header_table(name, "p")
    return [("p", pl, "U"), ("2 p, uncarried", [2 * x for x in pl], "U"),
            ("the subtraction pad", header_table(name, "subpad"), "mul input"),
            ("the largest multiple of p in U, top-heavy", top_heavy(0, p, U), "U")]


# ---- points ------------------------------------------------------------------------------------------------------------
# a point case: P = a G, Q = b G as raw limb vectors per coordinate; `what` says how each coordinate was written
Case = namedtuple("Case", "tag a b P Q what")
SEED = 0x5EED26
RANDOM_PAIRS = 10


def scalar_pairs(order, rng):
    """[(tag, a, b)]: Q = b G with b taken mod the order, so `order - b` is -b G"""
    a, b = rng.randrange(3, order), rng.randrange(3, order)
    out = [("a doubling", a, a), ("P + (-P)", a, order - a), ("the identity + Q", 0, b), ("P + the identity", a, 0),
           ("the identity twice", 0, 0), ("P - Q", a, order - b)]
    out += [("a = %s, b = %s" % (ta, tb), x, y) for ta, x in (("1", 1), ("2", 2), ("order - 1", order - 1))
            for tb, y in (("1", 1), ("2", 2), ("order - 1", order - 1))]
    out += [("random pair %d" % i, rng.randrange(3, order), rng.randrange(3, order)) for i in range(RANDOM_PAIRS)]
    return out


class ReprCases:
    def __init__(self, name):
        import ec_dual_cases
        self.name = name
        self.p = p = PRIMES[name]
        self.coords = COORDS[name]
        self.nc = len(self.coords)
        self.cs = cs = ec_dual_cases.cases(name)          # the oracle's results, cached there
        self.G, self.order, self.L = cs.G, cs.order, cs.L
        self.zeros = [("0", [0] * NLIMB, "U")] + zero_representatives(name)
        self.free = free_vectors(U)
        rng = random.Random(SEED + cs.gid)
        self.pairs = scalar_pairs(self.order, rng)
        self.cases = []
        for pi, (tag, a, b) in enumerate(self.pairs):
            for cp in range(self.nc):
                for fi in range(len(self.free)):
                    cq, fq = (cp + 1 + fi) % self.nc, (5 * fi + 3 + pi) % len(self.free)
                    P, wp = self.write_point(a, cp, fi, pi + cp + fi)
                    Q, wq = self.write_point(b, cq, fq, pi + cq + fq + 1)
                    self.cases.append(Case("%s; P: %s; Q: %s" % (tag, wp, wq), a, b, P, Q, (wp, wq)))

    # -- the oracle
    def enc(self, k):
        """the canonical encoding of k G"""
        k %= self.order
        return self.cs.ident if k == 0 else self.cs.mul(self.cs.gen, k)

    def affine(self, k):
        """k G as integers (x, y) from the oracle's encoding; None for the identity"""
        k %= self.order
        if k == 0:
            return None
        e = self.G.element_from_fixed(self.enc(k))
        return (e[0], e[1])

    # -- writing a point
    def rep(self, val, kind_index):
        reps = representatives(val, self.p, U)
        return reps[kind_index % len(reps)]

    def write_point(self, k, free_coord, free_index, rot):
        """k G with coordinate `free_coord` written as free vector `free_index` (the point scaled to fit) and the others
        as derived representatives, kinds rotating with `rot`.  The identity has one coordinate that may be anything
        (Y; ristretto255's Z is then forced to the same value); its zero coordinates rotate through the representatives of
        zero instead.  -> (list of limb vectors in the order of self.coords, description)"""
        p, names = self.p, self.coords
        ftag, fvec = self.free[free_index]
        f = value(fvec) % p
        assert f != 0
        xy = self.affine(k)
        if xy is None:
            zs = [self.zeros[(rot + j) % len(self.zeros)] for j in range(2)]
            derived = self.rep(f, rot)
            if names == "XYZ":
                vec = {"X": zs[0][1], "Y": fvec, "Z": zs[1][1]}
                what = "identity, Y = %s, X = %s, Z = %s" % (ftag, zs[0][0], zs[1][0])
            else:
                yz = (fvec, derived[1]) if free_coord % 2 == 0 else (derived[1], fvec)
                vec = {"X": zs[0][1], "Y": yz[0], "Z": yz[1], "T": zs[1][1]}
                what = "identity, %s = %s, the other %s, X = %s, T = %s" % ("YZ"[free_coord % 2], ftag, derived[0], zs[0][0], zs[1][0])
            return [vec[c] for c in names], what
        x, y = xy
        unit = {"X": x, "Y": y, "Z": 1, "T": x * y % p}            # the point at lambda = 1
        fc = names[free_coord]
        assert unit[fc] % p != 0
        lam = f * pow(unit[fc], -1, p) % p
        out, kinds = [], []
        for j, c in enumerate(names):
            if c == fc:
                out.append(fvec)
                continue
            kind, vec = self.rep(lam * unit[c] % p, rot + j)
            out.append(vec)
            kinds.append("%s %s" % (c, kind))
        return out, "%s = %s, %s" % (fc, ftag, ", ".join(kinds))

    def point_of(self, vectors):
        """the group element a list of limb vectors stands for, as the oracle's Python classes hold it"""
        p = self.p
        v = [value(x) % p for x in vectors]
        if self.name == "secp256k1":
            X, Y, Z = v
            if Z == 0:
                assert X == 0 and Y != 0
                return None
            zi = pow(Z, -1, p)
            return (X * zi % p, Y * zi % p)
        X, Y, Z, T = v
        assert Z != 0 and (T * Z - X * Y) % p == 0
        return (X, Y, Z, T)

    # -- expected scalars of what the unit programs compute
    def closure_scalar(self, a, b, steps=64):
        """acc <- acc + Q and acc <- 2 acc alternating, from acc = P"""
        k = a
        for s in range(steps):
            k = (k + b) % self.order if s % 2 == 0 else 2 * k % self.order
        return k

    def batches(self):
        """secp256k1's encode_batch<8>: [(tag, [(scalar, limb vectors)] * 8)] -- a weak-Z point, an identity written with
        a non-zero zero and ordinary points (Z = 1, canonical) in one batch, the identity first, last and in the middle"""
        assert self.name == "secp256k1"
        rng = random.Random(SEED + 8)
        out = []
        nz = len(self.zeros)
        for bi in range(4 * len(self.free)):
            fi, where = bi % len(self.free), (0, 7, 3, 4)[bi // len(self.free)]
            row = []
            for slot in range(8):
                k = rng.randrange(1, self.order)
                if slot == where:
                    z = 1 + (bi + slot) % (nz - 1)                     # never the plain 0
                    row.append((0, [self.zeros[(z + 1) % nz][1], self.free[(fi + 3) % len(self.free)][1], self.zeros[z][1]]))
                elif slot in ((where + 1) % 8, (where + 5) % 8):
                    row.append((k, self.write_point(k, 2, (fi + slot) % len(self.free), bi + slot)[0]))    # Z free
                elif slot == (where + 2) % 8:
                    row.append((k, self.write_point(k, slot % 2, fi, bi)[0]))                              # X or Y free
                else:
                    x, y = self.affine(k)
                    row.append((k, [limbs(x), limbs(y), limbs(1)]))
            out.append(("identity in slot %d, free vector %d" % (where, fi), row))
        return out


@functools.lru_cache(maxsize=None)
def repr_cases(name):
    return ReprCases(name)


# ---- what the unit programs compute (tests/ec_repr_ops.h) ---------------------------------------------------------------
SLOT_NAMES = ("add", "dbl", "neg", "add_affine +", "add_affine -", "add_cached +", "add_cached -", "cmov taken",
              "cmov not taken", "64 steps of add / dbl", "ks_is_identity")


def expected_slots(rc, case):
    """the encodings tests/ec_repr_ops.h documents for one case"""
    a, b = case.a, case.b
    aff = b if b % rc.order else 1                # an identity Q has no affine form: the generator stands in
    flags = bytes([(a % rc.order == 0) | (b % rc.order == 0) << 1]) + bytes(rc.L - 1)
    ks = (a + b, 2 * a, -a, a + aff, a - aff, a + b, a - b, b, a, rc.closure_scalar(a, b))
    return [rc.enc(k) for k in ks] + [flags]


def run_unit(exe, mode, blob, n, tmp_path):
    """a unit program of tests/_build on the GPU: one child under a time limit of its own; any non-zero status fails the
    test, nothing is tried again and nothing more is started.  -> the bytes it wrote"""
    import subprocess
    assert os.path.exists(exe), "build it with `make -C mpvss_rs_amd/csrc examples` (__graft_entry__.build() does)"
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    out = subprocess.run(["timeout", "-k", "10", "60", exe, str(mode), str(src), str(n), str(dst)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ran %d" % n), (mode, out.returncode, out.stdout[:600], out.stderr[-600:])
    return dst.read_bytes()


def words(vectors):
    """the u32 words of a point or of a list of points, little-endian"""
    flat = [x for v in vectors for x in v]
    return struct.pack("<%dI" % len(flat), *flat)
