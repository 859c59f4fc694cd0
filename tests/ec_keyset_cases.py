"""Cases for the key sets of the curve groups (csrc/ec_keyset.h): the keys, the edge scalars and the host shim that the CPU model
test (tests/test_ec_keyset_model.py) and the GPU tests (tests/test_gpu_ec_keyset.py) share.  Needs neither torch nor a GPU.

Expected values come from oracle/ec_ref.c (plain double-and-add) through ec_dual_cases.Cases.mul, which caches them."""
import ctypes as C
import functools
import os
import random
import subprocess

import ec_dual_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mpvss_rs_amd", "csrc")
WINDOWS, ENTRIES = 65, 8
ROW_BYTES = {"secp256k1": 33280, "ristretto255": 49920}       # 65 x 8 entries of 64 / 96 bytes
NIBBLES = (0x0, 0x7, 0x8, 0xF)


def load_shim():
    """tests/ec_keyset_host_shim.cpp as a shared library, built the way ec_dual_cases.load_shim builds its own"""
    lib = os.path.join(HERE, "_build", "libec_keyset_host.so")
    src = os.path.join(HERE, "ec_keyset_host_shim.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("ec_keyset.h", "ec_field.h", "ec_curves.h", "ec_consts.h")]
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        tmp = "%s.%d" % (lib, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", tmp])
        os.replace(tmp, lib)
    so = C.CDLL(lib)
    vp = C.c_void_p
    so.ks_row_words.argtypes = so.ks_entry_words.argtypes = [C.c_int]
    so.ks_build.argtypes = [C.c_int, vp, vp, vp, vp]
    so.ks_build.restype = None
    so.ks_walk.argtypes = [C.c_int, vp, C.c_int, vp, vp]
    so.ks_walk.restype = None
    so.ks_entry_encode.argtypes = [C.c_int, vp, vp]
    return so


@functools.lru_cache(maxsize=None)
def shim():
    return load_shim()


def entry_scalar(order, w, i):
    """the scalar of rows[key][w][i]"""
    return ((i + 1) << (4 * w)) % order


class KeysetCases:
    def __init__(self, name):
        self.name = name
        self.cs = cs = D.cases(name)
        self.gid, self.order, self.L = cs.gid, cs.order, cs.L
        rng = random.Random(0x5E7 + cs.gid)
        # G, the identity, -G, five random multiples
        self.keys = [cs.gen, cs.ident, cs.neg(cs.gen)] + [cs.mul(cs.gen, rng.randrange(2, cs.order)) for _ in range(5)]
        edge = [0, 1, 2, 8, 15, 16, cs.order - 1, cs.order - 2]
        self.unreachable = []
        for w in D.EXTREME_WINDOWS:
            for nib in NIBBLES:
                k = D.full_extreme(rng, cs.order, w, nib)
                if k is None:
                    self.unreachable.append((w, nib))      # (ristretto255: the order is just above 2^252, the top nibble stays small)
                else:
                    assert D.recoded_nibbles(k)[w] == nib
                    edge.append(k)
        self.top = []
        if name == "secp256k1":        # recoded window 64 is 1 from 0x77..78 on
            lo = int("7" * 63 + "8", 16)
            self.top = [lo, cs.order - 3] + [rng.randrange(lo, cs.order) for _ in range(3)]
            assert all(D.recoded_nibbles(k)[64] == 1 for k in self.top) and D.recoded_nibbles(lo - 1)[64] == 0
        self.edge = edge + self.top
        self.rng = rng

    def scalar(self, k):
        return self.cs.scalar(k)

    def mul(self, point, k):
        return self.cs.mul(point, k % self.order)

    def lane_scalars(self, n, seed):
        """n scalars: the edge list spread over the lanes (lane i holds an edge scalar when i = 3 mod 5), random elsewhere"""
        rng = random.Random(seed)
        out = []
        for i in range(n):
            out.append(self.edge[(i // 5 + seed) % len(self.edge)] if i % 5 == 3 else rng.randrange(self.order))
        return out

    def key_pool(self, n, seed):
        """n keys, all cheap for the reference: G, the identity and -G first, then small and random multiples of G"""
        rng = random.Random(seed)
        ks = list(self.keys[:3])
        while len(ks) < n:
            ks.append(self.cs.mul(self.cs.gen, rng.randrange(2, self.order)))
        return ks[:n]


@functools.lru_cache(maxsize=None)
def cases(name):
    return KeysetCases(name)
