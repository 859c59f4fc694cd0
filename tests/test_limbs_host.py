"""CPU unit tests of the MODP kernels' bytes <-> limbs edge: mpvss_rs_amd/csrc/modp_limbs.h is plain C++, so the very
functions the quad, pair and run-time kernels inline are compiled here with g++ (tests/limbs_host_shim.cpp) and compared
with Python integers: limb extraction from 256 big-endian bytes, the serial canonicalisation of an almost-normalised value
below 2N (with and without the scalar ring's parity lift) and the 32-bit words of the result."""
import ctypes as C
import os
import random
import subprocess

import pytest

import mpvss_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "liblimbs_host.so")
W = 29
MASK = (1 << W) - 1
LAZY = MASK + (1 << 9)          # the documented bound of an almost-normalised limb
RFC = O.ModpGroup().q


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(HERE, "limbs_host_shim.cpp")
    deps = [src, os.path.join(HERE, "..", "mpvss_rs_amd", "csrc", "modp_limbs.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", LIB])
    return C.CDLL(LIB)


def exact(v, L):
    assert v >> (W * L) == 0
    return [(v >> (W * j)) & MASK for j in range(L)]


def value(limbs):
    return sum(x << (W * j) for j, x in enumerate(limbs))


def test_be256_limb_all_72_limbs(shim):
    rng = random.Random(29)
    vals = [0, 1, RFC - 1, RFC, (1 << 2048) - 1, 1 << 2047, 0xFF << 2040, 1 << 2030, (1 << 2030) - 1, MASK << (W * 69)]
    vals += [1 << (W * j) for j in range(71)] + [rng.randrange(1 << 2048) for _ in range(50)]
    out = (C.c_uint32 * 72)()
    for v in vals:
        shim.limbs_from_be256((C.c_uint8 * 256).from_buffer_copy(v.to_bytes(256, "big")), out)
        assert list(out) == exact(v, 72), hex(v)
        assert out[70] < (1 << 18) and out[71] == 0


def lazy_vectors(N, L, rng):
    """limb vectors (every limb <= LAZY) of values below 2N whose carries are still pending"""
    t = (N.bit_length() - 1) // W                      # N's top limb
    out = []
    for pat in ("max", "mixed", "mixed", "mixed", "mask"):
        low = [LAZY if pat == "max" else MASK if pat == "mask" else rng.choice([0, 1, 511, MASK, MASK + 1, LAZY, rng.randrange(LAZY + 1)])
               for _ in range(t)]
        room = (2 * N - 1 - value(low)) >> (W * t)     # the largest top limb that keeps the value below 2N
        assert room >= 0
        for top in {min(room, LAZY), min(room, LAZY) // 2, 0}:
            out.append(low + [top] + [0] * (L - t - 1))
    return out


def moduli(L, rng):
    """odd moduli of a width of L limbs: one that fills the width's capacity (29 L - 2 bits, top limb in use), a short one"""
    cap = W * L - 2
    return [rng.randrange(1 << (cap - 1), 1 << cap) | 1, rng.randrange(1 << (cap - 40), 1 << (cap - 39)) | 1]


CASES = [(72, "rfc")] + [(L, "random") for L in (20, 36, 72, 10, 11, 21, 22)]


@pytest.mark.parametrize("L,kind", CASES)
def test_canonical_residue_and_words(shim, L, kind):
    """20 / 36 / 72 limbs are the library's widths; 10, 11, 21 and 22 are those at which a word of the result would need limb
    L or L + 1 (bit 32 wd = 29 (L - 2) + 27 or 29 (L - 2) + 28), which no shipped width reaches."""
    rng = random.Random(1000 + L)
    top = 1 << (W * (L - 1))
    for N in ([RFC] if kind == "rfc" else moduli(L, rng)):
        vecs = [exact(v, L) for v in (0, 1, 2, N - 1, N, N + 1, 2 * N - 1, 2 * N - 2, N - 2, N + 2)]
        # values that differ from N in the top limb alone, and in the top limb one way and below it the other way
        vecs += [exact(v, L) for v in (N - top, N + top, N + top - 1, N - top + 1) if 0 <= v < 2 * N and v >> (W * L) == 0]
        vecs += [exact(rng.randrange(2 * N), L) for _ in range(20)]
        vecs += lazy_vectors(N, L, rng)
        n_arr = (C.c_uint32 * L)(*exact(N, L))
        words = (C.c_uint32 * 64)()
        seen = set()
        for limbs in vecs:
            v = value(limbs)
            assert v < 2 * N and max(limbs) <= LAZY
            for lift in (-1, 0, 1):
                want = v % N
                if lift >= 0 and want % 2 != lift:
                    want += N
                seen.add((v >= N, lift, v % N % 2))
                slot = (C.c_uint32 * L)(*limbs)
                assert shim.limbs_canonical(L, slot, n_arr, lift, words) == 0
                assert list(slot) == exact(want, L), (L, hex(v), lift)
                assert list(words) == [(want >> (32 * wd)) & 0xFFFFFFFF for wd in range(64)], (L, hex(v), lift)
        assert len(seen) == 12          # reduced or not, no lift / even / odd, residue even or odd: all met


def test_unknown_width_is_refused(shim):
    assert shim.limbs_canonical(19, None, None, -1, None) == -1
