"""The decoders of mpvss_rs_amd/csrc/ec_curves.h (SEC1 compressed for secp256k1, RFC 9496 4.3.1 for ristretto255), compiled
with g++ (tests/ec_host_shim.cpp), against every classified vector of tests/encoding_vectors.py: each rejecting vector
fails exactly one decode check, so a decoder that dropped that check accepts it and this module turns red.  The same
vectors go through every decoding kernel on the GPU in tests/test_gpu_ec_encodings.py."""
import ctypes as C
import os
import random
import subprocess

import pytest

import encoding_vectors as EV
import mpvss_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "libec_host.so")
CURVES = [(0, "secp256k1"), (1, "ristretto255")]


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src = os.path.join(HERE, "ec_host_shim.cpp")
    deps = [src] + [os.path.join(HERE, "..", "mpvss_rs_amd", "csrc", f) for f in ("ec_field.h", "ec_curves.h", "ec_consts.h", "ec_glv.h", "ec_scalar.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", LIB])
    return C.CDLL(LIB)


def buf(b):
    return (C.c_uint8 * len(b)).from_buffer_copy(b)


@pytest.mark.parametrize("curve,name", CURVES)
def test_every_rejecting_vector_is_rejected(shim, curve, name):
    G = O.GROUPS[name]()
    bad = EV.rejecting(name)
    assert len(bad) >= 70
    out = (C.c_uint8 * G.elem_len)()
    good = G.element_to_bytes(G.generator())
    accepted = [label for label, b in bad if shim.ec_decode_ok(curve, buf(b)) != 0]
    assert accepted == []
    for label, b in bad:
        assert shim.ec_recode(curve, buf(b), out) == -1, label
        # the two operand positions of the addition and both points of the double multiplication
        assert shim.ec_add(curve, buf(b), buf(good), out, 0) == -1, label
        assert shim.ec_add(curve, buf(good), buf(b), out, 0) == -2, label
        assert shim.ec_dual(curve, buf(good), buf(G.scalar_to_bytes(1)), buf(b), buf(G.scalar_to_bytes(1)), out) == -2, label


@pytest.mark.parametrize("curve,name", CURVES)
def test_every_valid_vector_decodes_to_the_oracles_point(shim, curve, name):
    G = O.GROUPS[name]()
    rng = random.Random(0xE0C + curve)
    order = G.group_order_int()
    out = (C.c_uint8 * G.elem_len)()
    vs = EV.valid(name)
    assert len(vs) >= 36
    for label, b, pt in vs:
        assert shim.ec_decode_ok(curve, buf(b)) == 1, label
        assert shim.ec_recode(curve, buf(b), out) == 0 and bytes(out) == b, label
        for k in (1, 2, order - 1, rng.randrange(order)):
            assert shim.ec_dual(curve, buf(b), buf(G.scalar_to_bytes(k)), None, None, out) == 0
            assert bytes(out) == G.element_to_bytes(G.exp(pt, k)), (label, hex(k))
    # the identity's encoding is a valid input and is what the group law gives for P + (-P)
    ident = G.element_to_bytes(G.identity())
    assert (ident in [b for _, b, _ in vs]) and ident == bytes(G.elem_len)


def test_secp256k1_both_prefixes_are_opposite_points(shim):
    G = O.Secp256k1Group()
    out = (C.c_uint8 * 33)()
    by_x = {}
    for label, b, pt in EV.valid("secp256k1"):
        if any(b):
            by_x.setdefault(b[1:], {})[b[0]] = pt
    pairs = [(x, d) for x, d in by_x.items() if set(d) == {2, 3}]
    assert len(pairs) >= 34
    for x, d in pairs:
        assert d[2] != d[3] and d[2] == G.element_inverse(d[3])
        assert shim.ec_add(0, buf(b"\x02" + x), buf(b"\x03" + x), out, 0) == 0
        assert bytes(out) == bytes(33), x.hex()
        assert shim.ec_add(0, buf(b"\x02" + x), buf(b"\x02" + x), out, 0) == 0
        assert bytes(out) == G.element_to_bytes(G.mul(d[2], d[2])), x.hex()


def test_ristretto255_masked_aliases_are_rejected_not_folded(shim):
    """An encoding with bit 255 set, p + s0, and p - s0 each name a valid point for a decoder that masks, reduces or
    ignores the sign: the decoder must reject them AND must accept the canonical encoding they alias."""
    V = EV.vectors("ristretto255")
    p = EV.P25519
    for label, b, _ in V["bit255"]:
        alias = (int.from_bytes(b, "little") & ((1 << 255) - 1)).to_bytes(32, "little")
        assert shim.ec_decode_ok(1, buf(b)) == 0 and shim.ec_decode_ok(1, buf(alias)) == 1, label
    for label, b, _ in V["noncanonical"]:
        alias = (int.from_bytes(b, "little") - p).to_bytes(32, "little")
        assert shim.ec_decode_ok(1, buf(b)) == 0 and shim.ec_decode_ok(1, buf(alias)) == 1, label
    for label, b, _ in V["noncanonical+negative_s"]:
        alias = (2 * p - int.from_bytes(b, "little")).to_bytes(32, "little")     # p - s0
        assert shim.ec_decode_ok(1, buf(b)) == 0 and shim.ec_decode_ok(1, buf(alias)) == 1, label
    for label, b, _ in V["negative_s"]:
        alias = (p - int.from_bytes(b, "little")).to_bytes(32, "little")
        assert shim.ec_decode_ok(1, buf(b)) == 0 and shim.ec_decode_ok(1, buf(alias)) == 1, label
