"""Host side of a wide run-time MODP group (mpvss_modp_group_create_wide, 384-byte elements and scalars): what the handle
accepts and refuses, hash_to_scalar against the oracle, the scalar ring Z/(q-1) at 48 words against Python integers, and
the 384-byte bytes <-> limbs edge of the 27-limb kernels compiled for the CPU (tests/limbs_wide_host_shim.cpp).  No GPU."""
import ctypes as C
import os
import random
import subprocess

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
from mpvss_rs_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "liblimbs_wide_host.so")
EB, TOP = WH.EB, WH.TOP
W = 29
MASK = (1 << W) - 1
LAZY = MASK + (1 << 9)


@pytest.fixture(scope="module")
def grp15():
    g = capi.ModpGroup(WH.group15(), elem_bytes=EB)
    yield g
    g.close()


def test_create_wide_accepts_and_refuses():
    for q in (WH.group15(), WH.odd_2049()):
        g = capi.ModpGroup(q, elem_bytes=EB)
        assert (g.elem_bytes, g.limbs_per_lane, g.bits) == (384, 27, q.bit_length())
        g.close()
    refused = [(H.rfc_prime(2048), 384), ((1 << 2047) | 1, 384), ((1 << 3072) | 1, 384), (WH.group15() - 1, 384), (0, 384), (23, 384)]
    refused += [(WH.group15(), eb) for eb in (0, 255, 320, 512)] + [(H.rfc_prime(2048), eb) for eb in (0, 255, 320, 512)]
    for q, eb in refused:
        with pytest.raises(capi.EngineError):
            capi.ModpGroup(q, elem_bytes=eb)
    # the handles that exist today: 256 bytes, through either constructor, and still nothing above 2048 bits
    for g in (capi.ModpGroup(H.rfc_prime(2048)), capi.ModpGroup(H.rfc_prime(2048), elem_bytes=256), capi.ModpGroup(23, elem_bytes=256)):
        assert g.elem_bytes == 256 and g.limbs_per_lane in (5, 18)
        g.close()
    for eb in (None, 256):
        with pytest.raises(capi.EngineError):
            capi.ModpGroup(WH.group15()) if eb is None else capi.ModpGroup(WH.group15(), elem_bytes=eb)
    lib = capi.load_library()
    h = C.c_void_p()
    qb = bytes(5) + WH.group15().to_bytes(384, "big")              # leading zero bytes are allowed
    assert lib.mpvss_modp_group_create_wide(qb, len(qb), 384, C.byref(h)) == 0
    assert lib.mpvss_modp_group_elem_bytes(h) == 384 and lib.mpvss_modp_group_bits(h) == 3072
    lib.mpvss_modp_group_destroy(h)
    assert lib.mpvss_modp_group_create_wide(None, 0, 384, C.byref(h)) != 0
    assert lib.mpvss_modp_group_elem_bytes(None) < 0


def test_hash_to_scalar_against_the_oracle(grp15):
    g = H.RtOracleGroup(WH.group15())
    for data in (b"", b"abc", bytes(range(200))):
        out = grp15.hash_to_scalar(data)
        assert len(out) == EB and int.from_bytes(out, "big") == g.hash_to_scalar(data)
    # a real reduction needs (q-1)/2 below 2^256, which no wide modulus has: the padding is what is checked here
    assert grp15.hash_to_scalar(b"abc")[:EB - 32] == bytes(EB - 32)


def _operands(q, rng):
    return [q - 2, 0, 1, q - 1, q, TOP, rng.randrange(q - 1, 1 << 3072), rng.randrange(q - 1), rng.getrandbits(3072), rng.getrandbits(2049)]


@pytest.mark.parametrize("which", ["group15", "odd2049"])
def test_scalar_ring_against_python_ints(which):
    q = WH.group15() if which == "group15" else WH.odd_2049()
    grp = capi.ModpGroup(q, elem_bytes=EB)
    rng = random.Random(q & 0xFFFF)
    ops = _operands(q, rng)
    checked_sub = 0
    for a in ops:
        for b in ops:
            assert int.from_bytes(capi.group_scalar_mul(grp, WH.be(a), WH.be(b)), "big") == a * b % (q - 1)
            d = a - b
            want = d + (q - 1) if d < 0 else d % (q - 1)          # modp.rs:184-192
            if want >= 0:                                         # a - b + (q-1) < 0 has no BigUint encoding in the reference
                assert int.from_bytes(capi.group_scalar_sub(grp, WH.be(a), WH.be(b)), "big") == want
                checked_sub += 1
    assert checked_sub >= len(ops) * (len(ops) + 1) // 2
    # r_i = w_i - alpha_i c mod (q-1), shared and per-share c
    n = len(ops)
    ws, als = ops, ops[::-1]
    for c in (0, 1, q - 2, TOP, rng.getrandbits(256)):
        got = WH.split(capi.group_dleq_responses(grp, WH.cat(ws), WH.cat(als), WH.be(c)))
        assert got == [(w - al * c) % (q - 1) for w, al in zip(ws, als)]
    cs = [rng.getrandbits(3072) for _ in range(n)]
    got = WH.split(capi.group_dleq_responses(grp, WH.cat(ws), WH.cat(als), WH.cat(cs)))
    assert got == [(w - al * c) % (q - 1) for w, al, c in zip(ws, als, cs)]
    # P(i) mod (q-1): t = 1, 2, 17, positions 1, 2, 33 among others, and a run long enough for the difference table
    for t in (1, 2, 17):
        coeffs = ([q - 2, 0, TOP] + [rng.getrandbits(3072) for _ in range(t)])[:t]
        for positions in ([1, 2, 33], [0, 33, 2, 1, (1 << 62) + 5], list(range(1, 4 * t + 8))):
            got = WH.split(capi.group_poly_eval(grp, WH.cat(coeffs), positions, threads=2))
            assert got == [sum(c * i ** j for j, c in enumerate(coeffs)) % (q - 1) for i in positions]
    grp.close()


def test_a_256_byte_handle_is_untouched_by_the_wide_one():
    """both sizes side by side in one process: each handle answers at its own stride"""
    q14 = H.rfc_prime(2048)
    narrow, wide = capi.ModpGroup(q14), capi.ModpGroup(WH.group15(), elem_bytes=EB)
    a, b = q14 - 2, (1 << 2048) - 1
    for _ in range(2):
        assert capi.group_scalar_mul(narrow, WH.be(a, 256), WH.be(b, 256)) == WH.be(a * b % (q14 - 1), 256)
        assert capi.group_scalar_mul(wide, WH.be(a), WH.be(b)) == WH.be(a * b % (WH.group15() - 1))
        assert len(narrow.hash_to_scalar(b"x")) == 256 and len(wide.hash_to_scalar(b"x")) == 384
    narrow.close()
    wide.close()


# ---- the byte edge on the CPU ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(HERE, "limbs_wide_host_shim.cpp")
    deps = [src, os.path.join(HERE, "..", "mpvss_rs_amd", "csrc", "modp_limbs.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", LIB])
    return C.CDLL(LIB)


def exact(v, L=108):
    assert v >> (W * L) == 0
    return [(v >> (W * j)) & MASK for j in range(L)]


def lazy_limbs(v, rng, L=108):
    """v in almost-normalised limbs: some limbs carry up to 2^9 extra units borrowed from the limb above"""
    l = exact(v, L)
    for j in range(L - 1):
        k = min(l[j + 1], rng.randrange(2))
        if k and l[j] + (k << W) <= LAZY:
            l[j] += k << W
            l[j + 1] -= k
    assert sum(x << (W * j) for j, x in enumerate(l)) == v and max(l) <= LAZY
    return l


def test_be_limb_384_all_108_limbs(shim):
    rng = random.Random(384)
    q = WH.group15()
    vals = [0, 1, q - 1, q, TOP, 1 << 3071, 0xFF << 3064, 1 << 2048, (1 << 2048) - 1] + [1 << (W * j) for j in range(106)]
    vals += [rng.randrange(1 << 3072) for _ in range(30)]
    out = (C.c_uint32 * 108)()
    for v in vals:
        shim.limbs_from_be384(WH.be(v), out)
        assert list(out) == exact(v), hex(v)
        assert out[106] == 0 and out[107] == 0 and out[105] < (1 << (3072 - W * 105))


@pytest.mark.parametrize("which", ["group15", "top", "odd2049"])
def test_canonicalize_and_words_at_108_limbs(shim, which):
    N = {"group15": WH.group15(), "top": TOP, "odd2049": WH.odd_2049()}[which]
    rng = random.Random(108)
    n = (C.c_uint32 * 108)(*exact(N))
    words = (C.c_uint32 * 96)()
    vals = [0, 1, N - 1, N, N + 1, 2 * N - 1, min(TOP, 2 * N - 1)] + [rng.randrange(2 * N) for _ in range(20)]
    for v in vals:
        for limbs_in in (exact(v), lazy_limbs(v, rng)):
            slot = (C.c_uint32 * 108)(*limbs_in)
            shim.limbs_canonical108(slot, n, words)
            want = v - N if v >= N else v
            assert list(slot) == exact(want), (which, hex(v))
            assert sum(w << (32 * i) for i, w in enumerate(words)) == want
