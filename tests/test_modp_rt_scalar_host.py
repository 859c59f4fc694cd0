"""The scalar ring Z/(q-1) of a run-time MODP group on the host (mpvss_modp_group_scalar_mul / _scalar_sub / _poly_eval /
_dleq_responses) against the oracle over tests/modp_rt_helpers.RtOracleGroup(q): moduli from 3 to 2048 bits, operands that
are not reduced, and byte identity with the group-14 functions for the RFC 3526 prime.  No GPU."""
import random

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
from mpvss_rs_amd import ModpGroup, capi

EB = 256
TOP = (1 << 2048) - 1


def enc(v):
    return v.to_bytes(EB, "big")


def cat(vals):
    return b"".join(enc(v) for v in vals)


def split(b):
    return [int.from_bytes(b[i:i + EB], "big") for i in range(0, len(b), EB)]


def _moduli():
    rng = random.Random(2048)
    sp = H.small_safe_primes()
    out = [5, 23, sp[40], sp[64], sp[256]]
    out += [H.rfc_prime(k) for k in (768, 1024, 1536, 2048)]
    out += [H.random_odd_modulus(2047, rng), H.random_odd_modulus(2048, rng)]
    return out


MODULI = _moduli()
IDS = [f"{q.bit_length()}b" for q in MODULI]


def _operands(q, rng, extra=6):
    ops = [0, 1, q - 2, q - 1, q, TOP]
    ops += [rng.randrange(q) for _ in range(extra)]
    ops += [rng.randrange(1 << 2048) for _ in range(extra)]
    return ops


@pytest.mark.parametrize("q", MODULI, ids=IDS)
def test_scalar_mul_and_sub_match_the_oracle(q):
    g, grp = H.RtOracleGroup(q), ModpGroup(q)
    rng = random.Random(q & 0xFFFF)
    ops = _operands(q, rng)
    checked_sub = 0
    for a in ops:
        for b in ops:
            assert split(capi.group_scalar_mul(grp, enc(a), enc(b))) == [g.scalar_mul(a, b)], (a, b)
            want = g.scalar_sub(a, b)
            if want >= 0:            # a - b + (q-1) < 0 has no BigUint encoding in the reference
                assert split(capi.group_scalar_sub(grp, enc(a), enc(b))) == [want], (a, b)
                checked_sub += 1
    assert checked_sub > len(ops)


@pytest.mark.parametrize("q", MODULI, ids=IDS)
@pytest.mark.parametrize("t", [1, 40])
def test_poly_eval_matches_the_oracle(q, t):
    g, grp = H.RtOracleGroup(q), ModpGroup(q)
    rng = random.Random(t * 7 + (q & 0xFFF))
    coeffs = [rng.randrange(q - 1) for _ in range(t)]
    for k, v in enumerate((0, 1, q - 2, q - 1, q, TOP)):        # edge coefficients, not reduced
        if k < t:
            coeffs[k] = v
    # 0, 1, 2^62, a long consecutive run (the forward-difference path of the shared body) and random ones
    positions = [0, 1, 1 << 62] + list(range(1, 4 * t + 40)) + [rng.randrange(1 << 62) for _ in range(5)]
    want = [O.poly_get_value(coeffs, x) % (q - 1) for x in positions]
    one = capi.group_poly_eval(grp, cat(coeffs), positions, threads=1)
    assert split(one) == want
    assert capi.group_poly_eval(grp, cat(coeffs), positions, threads=7) == one


@pytest.mark.parametrize("q", MODULI, ids=IDS)
def test_dleq_responses_match_the_oracle(q):
    g, grp = H.RtOracleGroup(q), ModpGroup(q)
    rng = random.Random(q & 0xFFFFF)
    n = 300                                                      # above the threading threshold of parallel_for
    edge = [0, 1, q - 2, q - 1, q, TOP]
    w = [edge[i % 6] if i < 36 else rng.randrange(1 << rng.choice((q.bit_length(), 2048))) for i in range(n)]
    alpha = [edge[(i // 6) % 6] if i < 36 else rng.randrange(1 << rng.choice((q.bit_length(), 2048))) for i in range(n)]
    cs = [edge[i % 6] if i < 6 else rng.randrange(max(g.g, 1)) for i in range(n)]
    # one shared challenge
    for c in (0, 1, cs[7], q, TOP):
        want = [O.dleq_response(g, w[i], alpha[i], c) for i in range(n)]
        one = capi.group_dleq_responses(grp, cat(w), cat(alpha), enc(c), threads=1)
        assert split(one) == want
        assert capi.group_dleq_responses(grp, cat(w), cat(alpha), enc(c), threads=7) == one
    # one challenge per share
    want = [O.dleq_response(g, w[i], alpha[i], cs[i]) for i in range(n)]
    one = capi.group_dleq_responses(grp, cat(w), cat(alpha), cat(cs), threads=1)
    assert split(one) == want
    assert capi.group_dleq_responses(grp, cat(w), cat(alpha), cat(cs), threads=7) == one


def test_group14_scalar_ring_is_byte_identical_through_the_runtime_handle():
    q = H.rfc_prime(2048)
    assert q == O.ModpGroup().q
    grp = ModpGroup(q)
    rng = random.Random(14)
    ops = _operands(q, rng, extra=4)
    for a in ops:
        for b in ops:
            assert capi.group_scalar_mul(grp, enc(a), enc(b)) == capi.scalar_mul(0, enc(a), enc(b))
            assert capi.group_scalar_sub(grp, enc(a), enc(b)) == capi.scalar_sub(0, enc(a), enc(b))
    for t in (1, 40):
        coeffs = cat([rng.randrange(1 << 2048) for _ in range(t)])
        positions = [0, 1, 1 << 62] + list(range(1, 4 * t + 20))
        assert capi.group_poly_eval(grp, coeffs, positions, threads=3) == capi.poly_eval(0, coeffs, positions, threads=3)
    n = 280
    w = cat([rng.randrange(1 << 2048) for _ in range(n)])
    alpha = cat([rng.randrange(1 << 2048) for _ in range(n)])
    c1 = enc(rng.randrange(1 << 256))
    cn = cat([rng.randrange(1 << 2048) for _ in range(n)])
    for c in (c1, cn):
        assert capi.group_dleq_responses(grp, w, alpha, c, threads=4) == capi.dleq_responses(0, w, alpha, c, threads=4)


def test_hash_to_scalar_still_matches_the_oracle():
    """the handle's hash_to_scalar moved from bit-serial doubling to the word arithmetic of the scalar ring"""
    for q in MODULI:
        g, grp = H.RtOracleGroup(q), ModpGroup(q)
        for data in (b"", b"abc", bytes(range(64))):
            assert int.from_bytes(grp.hash_to_scalar(data), "big") == g.hash_to_scalar(data)


def test_bad_arguments():
    grp = ModpGroup(23)
    lib = grp.lib
    assert lib.mpvss_modp_group_scalar_mul(None, None, None, None) == -1
    assert lib.mpvss_modp_group_poly_eval(grp.handle, None, 0, None, 0, None, 1) == 0          # n == 0
    with pytest.raises(capi.EngineError):
        capi.group_poly_eval(grp, enc(1), [-1])
    with pytest.raises(capi.EngineError):
        capi.group_poly_eval(grp, b"", [1])                                                    # t == 0
