"""Host side of the Fiat-Shamir transcript at its byte edges (mpvss_rs_amd/csrc/sha256.cpp and the framers behind
mpvss_modp_transcript_absorb / mpvss_ec_transcript_absorb) against hashlib: every message length 0 ... 300, element streams whose
running length visits every residue mod 64 (SHA-256 padding spills into a further block at 56 ... 63), absorbed at once, one
element per call, and split at every element boundary.

The library picks its compression function once, at load time (SHA-NI when the CPU has it) and has no switch for the other one;
the portable function is covered by compiling sha256.cpp on its own with the x86 branch preprocessed away
(tests/sha256_host_shim.cpp).  The framers themselves run over whichever function the library picked on this machine."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import mpvss_oracle as O
from mpvss_rs_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "libsha256_portable.so")
EB = 256


def msg(n, salt=0):
    return bytes((i * 131 + n * 7 + salt) & 0xFF for i in range(n))


def test_library_sha256_every_length_to_300():
    for n in range(301):
        d = msg(n)
        assert capi.sha256(d) == hashlib.sha256(d).digest(), n


@pytest.fixture(scope="module")
def portable():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(HERE, "sha256_host_shim.cpp")
    deps = [src] + [os.path.join(HERE, "..", "mpvss_rs_amd", "csrc", f) for f in ("sha256.cpp", "sha256.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.portable_sha256_split.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.portable_sha256_split.restype = None
    return lib


def test_portable_sha256_every_length_and_cut(portable):
    assert portable.portable_uses_shani() == 0
    out = (C.c_uint8 * 32)()
    for n in range(301):
        d = msg(n, 3)
        want = hashlib.sha256(d).digest()
        b = (C.c_uint8 * max(n, 1)).from_buffer_copy(d or b"\0")
        for cut in sorted({0, n // 3, n // 2, max(n - 1, 0), n} | {c for c in (1, 55, 56, 63, 64, 65, 119, 128) if c <= n}):
            portable.portable_sha256_split(b, n, cut, out)
            assert bytes(out) == want, (n, cut)


_lib = capi.load_library()           # capi's helpers load and re-declare the library on every call: too slow for ~20 000 absorbs


def absorb(group, state, elements, width):
    """capi.transcript_absorb / capi.ec_transcript_absorb (group None: MODP) over the library handle made once"""
    st = C.create_string_buffer(bytes(state), len(state))
    buf = C.create_string_buffer(elements or b"\0", max(len(elements), 1))
    n = len(elements) // width
    rc = _lib.mpvss_modp_transcript_absorb(st, buf, n) if group is None else _lib.mpvss_ec_transcript_absorb(group, st, buf, n)
    assert rc == 0
    return st.raw


def verdict(group, state, challenge):
    """(verdict, digest) as capi.transcript_verdict / capi.ec_transcript_verdict give it"""
    st = C.create_string_buffer(bytes(state), len(state))
    ch = C.create_string_buffer(challenge, len(challenge))
    out = C.create_string_buffer(32)
    v = C.c_int(-1)
    rc = _lib.mpvss_modp_transcript_verdict(st, ch, C.byref(v), out) if group is None else \
        _lib.mpvss_ec_transcript_verdict(group, st, ch, C.byref(v), out)
    assert rc == 0 and v.value in (0, 1)
    return bool(v.value), out.raw


def modp_streams():
    """element streams (ints) whose framed running length visits every residue mod 64 at an element boundary: element lengths 1 (values
    0 and 1), 2 ... 5, 55 ... 57, 63 ... 65, 119 ... 121, 252 ... 256, values >= q, every leading-byte position inside a word"""
    rng = random.Random(0x7A)
    q = O.ModpGroup().q
    streams = []
    for base in range(8):
        lens = [1, 1] + [((base * 37 + k * 11) % 256) + 1 for k in range(40)] + [2, 3, 4, 5, 55, 56, 57, 63, 64, 65, 119, 120, 121,
                                                                                252, 253, 254, 255, 256]
        rng.shuffle(lens)
        elems = []
        for k, ln in enumerate(lens):
            if ln == 1:
                elems.append((0, 1, 0x80, 0xFF)[k % 4])
            elif ln == 256 and k % 2:
                elems.append(q + rng.randrange(1 << 1900))
            else:
                elems.append(rng.randrange(1 << (8 * ln - 8), 1 << (8 * ln)))
        streams.append(elems)
    return streams


def test_modp_framer_every_residue_three_ways():
    g = O.ModpGroup()
    init = capi.transcript_init()
    seen = set()
    for elems in modp_streams():
        raw = b"".join(e.to_bytes(EB, "big") for e in elems)
        framed = [O.framed(g.element_to_bytes(e)) for e in elems]
        total = 0
        for f in framed:
            total += len(f)
            seen.add(total % 64)
        digest = hashlib.sha256(b"".join(framed)).digest()
        c = hashlib.sha256(digest).digest().rjust(EB, b"\0")
        wrong = bytearray(c); wrong[-1] ^= 1
        st = capi.transcript_absorb(capi.transcript_init(), raw)
        assert capi.transcript_verdict(st, c) == (True, digest)
        assert capi.transcript_verdict(st, bytes(wrong)) == (False, digest)
        st = capi.transcript_init()
        for k in range(len(elems)):
            st = capi.transcript_absorb(st, raw[k * EB:(k + 1) * EB])
        assert capi.transcript_verdict(st, c) == (True, digest)
        for k in range(len(elems) + 1):
            st = absorb(None, absorb(None, init, raw[:k * EB], EB), raw[k * EB:], EB)
            assert verdict(None, st, c) == (True, digest), k
    assert seen == set(range(64))


@pytest.mark.parametrize("name", ["secp256k1", "ristretto255"])
def test_ec_framer_1_to_130_elements_three_ways(name):
    G = O.GROUPS[name]()
    gid = {"secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}[name]
    L = G.elem_len
    rng = random.Random(0x7B + L)
    blob = bytes(rng.randrange(256) for _ in range(130 * L))       # the framer hashes the bytes as given
    seen = set()
    init = capi.transcript_init()
    for n in range(1, 131):
        raw = blob[:n * L]
        framed = b"".join(O.framed(raw[k * L:(k + 1) * L]) for k in range(n))
        seen.add(len(framed) % 64)
        digest = hashlib.sha256(framed).digest()
        c = G.scalar_to_bytes(G.hash_to_scalar(digest))
        st = capi.ec_transcript_absorb(gid, capi.transcript_init(), raw)
        assert capi.ec_transcript_verdict(gid, st, c) == (True, digest), n
        wrong = bytearray(c); wrong[5] ^= 4
        assert capi.ec_transcript_verdict(gid, st, bytes(wrong))[0] is False
        st = init
        for k in range(n):
            st = absorb(gid, st, raw[k * L:(k + 1) * L], L)
        assert capi.ec_transcript_verdict(gid, st, c) == (True, digest), n
        for k in range(n + 1):
            st = absorb(gid, absorb(gid, init, raw[:k * L], L), raw[k * L:], L)
            assert verdict(gid, st, c) == (True, digest), (n, k)
    assert len(seen) == (64 if L == 33 else 8)        # 41 n mod 64 visits every residue, 40 n the multiples of 8
