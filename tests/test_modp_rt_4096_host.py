"""Host side of a 512-byte run-time MODP group (mpvss_modp_group_create_wide with elem_bytes 512, moduli of 3073 .. 4096 bits):
what the handle accepts and refuses, hash_to_scalar against the oracle, and the scalar ring Z/(q-1) at 64 words against Python
integers at the edges q - 2, 0, 1, q - 1, q, 2^4096 - 1.  Follows tests/test_modp_rt_wide_host.py.  Also holds the oracle's
protocol run of the GPU tests (XH.protocol_run, libcrypto under the oracle's exp) to Python's own pow on a sample.  No GPU."""
import ctypes as C
import hashlib
import random

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import modp_rt_4096_helpers as XH
import mpvss_oracle as O
from mpvss_rs_amd import capi

EB, TOP = XH.EB, XH.TOP


@pytest.fixture(scope="module")
def grp16():
    g = capi.ModpGroup(XH.group16(), elem_bytes=EB)
    yield g
    g.close()


def test_create_wide_accepts_and_refuses_at_512_bytes():
    for q in (XH.group16(), XH.odd_3073(), TOP):
        g = capi.ModpGroup(q, elem_bytes=EB)
        assert (g.elem_bytes, g.limbs_per_lane, g.bits) == (512, 36, q.bit_length())
        g.close()
    # a narrower q (the 256- or 384-byte handle serves it), 4097 bits, an even q, no q
    refused = [(WH.group15(), 512), (H.rfc_prime(2048), 512), ((1 << 3071) | 1, 512), ((1 << 4096) | 1, 512), (XH.group16() - 1, 512), (0, 512),
               (23, 512)]
    refused += [(XH.group16(), eb) for eb in (0, 256, 384, 448, 511, 640, 1024)]
    for q, eb in refused:
        with pytest.raises(capi.EngineError):
            capi.ModpGroup(q, elem_bytes=eb)
    lib = capi.load_library()
    h = C.c_void_p()
    qb = bytes(5) + XH.group16().to_bytes(512, "big")              # leading zero bytes are allowed
    assert lib.mpvss_modp_group_create_wide(qb, len(qb), 512, C.byref(h)) == 0
    assert lib.mpvss_modp_group_elem_bytes(h) == 512 and lib.mpvss_modp_group_bits(h) == 4096
    assert lib.mpvss_modp_group_limbs_per_lane(h) == 36
    lib.mpvss_modp_group_destroy(h)
    assert lib.mpvss_modp_group_create_wide(qb, len(qb), 640, C.byref(h)) != 0
    assert lib.mpvss_modp_group_create_wide(None, 0, 512, C.byref(h)) != 0


def test_the_handle_reports_its_sizes(grp16):
    assert grp16.keyset_bytes_per_key == 16 * 16 * 144 * 4 == 147456
    assert grp16.has_device_scalar and grp16.has_device_share_hash          # q = 7 mod 8, (q-1)/2 >= 2^256
    narrow = capi.ModpGroup(H.rfc_prime(2048))
    assert (grp16.twin_min_shares, grp16.comb_min_shares) == (narrow.twin_min_shares, narrow.comb_min_shares)
    narrow.close()


def test_hash_to_scalar_against_the_oracle(grp16):
    g = H.RtOracleGroup(XH.group16())
    for data in (b"", b"abc", bytes(range(200))):
        out = grp16.hash_to_scalar(data)
        assert len(out) == EB and int.from_bytes(out, "big") == g.hash_to_scalar(data)
    assert grp16.hash_to_scalar(b"abc")[:EB - 32] == bytes(EB - 32)


def _operands(q, rng):
    return [q - 2, 0, 1, q - 1, q, TOP, rng.randrange(q - 1, 1 << 4096), rng.randrange(q - 1), rng.getrandbits(4096), rng.getrandbits(3073)]


@pytest.mark.parametrize("which", ["group16", "odd3073", "top"])
def test_scalar_ring_against_python_ints(which):
    q = {"group16": XH.group16(), "odd3073": XH.odd_3073(), "top": TOP}[which]
    grp = capi.ModpGroup(q, elem_bytes=EB)
    rng = random.Random(q & 0xFFFF)
    ops = _operands(q, rng)
    checked_sub = 0
    for a in ops:
        for b in ops:
            assert int.from_bytes(capi.group_scalar_mul(grp, XH.be(a), XH.be(b)), "big") == a * b % (q - 1)
            d = a - b
            want = d + (q - 1) if d < 0 else d % (q - 1)          # modp.rs:184-192
            if want >= 0:                                         # a - b + (q-1) < 0 has no BigUint encoding in the reference
                assert int.from_bytes(capi.group_scalar_sub(grp, XH.be(a), XH.be(b)), "big") == want
                checked_sub += 1
    assert checked_sub >= len(ops) * (len(ops) + 1) // 2
    # r_i = w_i - alpha_i c mod (q-1), shared and per-share c
    n = len(ops)
    ws, als = ops, ops[::-1]
    for c in (0, 1, q - 2, TOP, rng.getrandbits(256)):
        got = XH.split(capi.group_dleq_responses(grp, XH.cat(ws), XH.cat(als), XH.be(c)))
        assert got == [(w - al * c) % (q - 1) for w, al in zip(ws, als)]
    cs = [rng.getrandbits(4096) for _ in range(n)]
    got = XH.split(capi.group_dleq_responses(grp, XH.cat(ws), XH.cat(als), XH.cat(cs)))
    assert got == [(w - al * c) % (q - 1) for w, al, c in zip(ws, als, cs)]
    # P(i) mod (q-1): t = 1, 2, 17, positions 1, 2, 33 among others, and a run long enough for the difference table
    for t in (1, 2, 17):
        coeffs = ([q - 2, 0, TOP] + [rng.getrandbits(4096) for _ in range(t)])[:t]
        for positions in ([1, 2, 33], [0, 33, 2, 1, (1 << 62) + 5], list(range(1, 4 * t + 8))):
            got = XH.split(capi.group_poly_eval(grp, XH.cat(coeffs), positions, threads=2))
            assert got == [sum(c * i ** j for j, c in enumerate(coeffs)) % (q - 1) for i in positions]
    grp.close()


def test_three_handle_sizes_side_by_side_on_the_host():
    """256, 384 and 512 bytes in one process: each handle answers at its own stride"""
    q14, q15, q16 = H.rfc_prime(2048), WH.group15(), XH.group16()
    groups = [(capi.ModpGroup(q14), q14, 256), (capi.ModpGroup(q15, elem_bytes=384), q15, 384), (capi.ModpGroup(q16, elem_bytes=512), q16, 512)]
    for _ in range(2):
        for grp, q, eb in groups:
            a, b = q - 2, (1 << (8 * eb)) - 1
            assert capi.group_scalar_mul(grp, XH.be(a, eb), XH.be(b, eb)) == XH.be(a * b % (q - 1), eb)
            assert len(grp.hash_to_scalar(b"x")) == eb
    for grp, _, _ in groups:
        grp.close()


def test_the_oracle_s_run_over_libcrypto_is_the_run_over_pow():
    """XH.protocol_run lets the oracle exponentiate through libcrypto where it can: what it returns at (5, 3) follows from its
    inputs by hashing, integer arithmetic and Python's own pow (one share's elements, 8 pows of 4096 bits)"""
    n, t = 5, 3
    G = XH.protocol_run(n, t)
    g = H.RtOracleGroup(XH.group16())
    q, privs, coeffs, ws, w2 = g.q, G["privs"], G["coeffs"], G["ws"], G["w2"]
    h = hashlib.sha256()
    for row in zip(G["X"], G["Y"], G["a1"], G["a2"]):
        h.update(O.append_transcript(g, *row))
    assert h.digest() == G["digest"] and g.hash_to_scalar(G["digest"]) == G["challenge"]
    P = [O.poly_get_value(coeffs, i) % (q - 1) for i in range(1, n + 1)]
    assert G["responses"] == [(w - p * G["challenge"]) % (q - 1) for w, p in zip(ws, P)]
    assert G["share_response"] == [(w - k * c) % (q - 1) for w, k, c in zip(w2, privs, G["share_challenge"])]
    assert {s for _, s in G["reconstructed"]} == {XH.SECRET} and G["tampered_valid"] is False
    i = n // 2
    assert G["pks"][i] == pow(2, privs[i], q) and G["commitments"][t - 1] == pow(4, coeffs[t - 1], q)
    assert G["Y"][i] == pow(G["pks"][i], P[i], q)
    assert (G["a1"][i], G["a2"][i]) == (pow(4, ws[i], q), pow(G["pks"][i], ws[i], q))
    assert G["share"][i] == pow(G["Y"][i], O.mod_inverse(privs[i], q - 1), q)
    a1, a2 = pow(2, w2[i], q), pow(G["share"][i], w2[i], q)
    assert g.hash_to_scalar(hashlib.sha256(O.append_transcript(g, G["pks"][i], G["Y"][i], a1, a2)).digest()) == G["share_challenge"][i]
