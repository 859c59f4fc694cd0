"""Run-time MODP groups (ModpGroup::init, src/groups/modp.rs:72-84) on the GPU: exp / mul against Python's pow at every width
boundary and for edge operands, group 14 through the run-time path against the group-14 entry points, and the protocol
(verify_distribution, verify_shares) against the oracle at 64 .. 1536 bits."""
import random
import threading

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
from helpers import make_modp_instance
from mpvss_rs_amd import ModpGroup

pytestmark = pytest.mark.gpu

EB = 256


def enc(v):
    return (v % (1 << 2048)).to_bytes(EB, "big")


def cat(vals):
    return b"".join(enc(v) for v in vals)


def split(b):
    return [int.from_bytes(b[i:i + EB], "big") for i in range(0, len(b), EB)]


def _moduli():
    rng = random.Random(11)
    out = []
    for bits in (578, 579, 1042, 1043, 2047, 2048):
        q = H.random_odd_modulus(bits, rng)
        while q % (1 << 29) == (1 << 29) - 1:     # keep n0inv != 1 for these
            q = H.random_odd_modulus(bits, rng)
        out.append(q)
    for k in (64, 580, 1044, 2048):
        out.append(2 ** k - 1)                     # all-ones limbs
        out.append(2 ** (k - 1) + 1)
    out += [H.rfc_prime(1024), H.small_safe_primes()[64], 5, 23]
    return out


MODULI = _moduli()


def _edge_cases(q, n, rng):
    bases = [b for b in (0, 1, q - 1, q, q + 1) if b < (1 << 2048)] + [(1 << 2048) - 1]
    exps = [0, 1, max(q - 2, 0), (1 << 2048) - 1]
    B, E = [], []
    for b in bases:
        for e in exps:
            B.append(b)
            E.append(e)
    while len(B) < n:
        B.append(rng.randrange(1 << min(2048, q.bit_length() + 8)))
        E.append(rng.randrange(1 << rng.choice((1, 64, q.bit_length(), 2048))))
    return B[:n], E[:n]


@pytest.mark.parametrize("q", MODULI, ids=[f"{q.bit_length()}b" for q in MODULI])
def test_batch_exp_and_mul_match_python(engine, q):
    grp = ModpGroup(q)
    assert grp.bits == q.bit_length() and grp.limbs_per_lane == H.width_for_bits(q.bit_length())
    rng = random.Random(q & 0xFFFF)
    for n in (1, 17, 33):
        B, E = _edge_cases(q, n, rng)
        got = split(engine.group_batch_exp(grp, cat(B), cat(E)))
        assert got == [pow(b, e, q) for b, e in zip(B, E)], (q.bit_length(), n)
        A = list(reversed(B))
        got = split(engine.group_batch_mul(grp, cat(A), cat(B)))
        assert got == [(a * b) % q for a, b in zip(A, B)]


@pytest.mark.parametrize("n", [15, 4097])
def test_ragged_batches(engine, n):
    rng = random.Random(n)
    for q in (H.rfc_prime(768), H.random_odd_modulus(1500, rng)):
        grp = ModpGroup(q)
        B = [rng.randrange(1 << 2048) for _ in range(n)]
        E = [rng.randrange(1 << rng.choice((8, 300, 2048))) for _ in range(n)]
        got = split(engine.group_batch_exp(grp, cat(B), cat(E)))
        idx = list(range(0, n, max(1, n // 200))) + [n - 1]
        assert [got[i] for i in idx] == [pow(B[i], E[i], q) for i in idx]


def test_group14_through_the_runtime_path_is_byte_identical(engine):
    g, privs, pks, coeffs, ws, box = make_modp_instance(9, 4, seed=77)
    grp = ModpGroup(g.q)
    assert grp.limbs_per_lane == 18
    rng = random.Random(3)
    B = [rng.randrange(1 << 2048) for _ in range(40)] + [0, 1, g.q, g.q + 1]
    E = [rng.randrange(1 << 2048) for _ in range(40)] + [5, 0, 7, (1 << 2048) - 1]
    assert engine.group_batch_exp(grp, cat(B), cat(E)) == engine.batch_exp(cat(B), cat(E))
    flat = O.box_to_flat(g, box)
    pos = flat["positions"] + [0, 1 << 40]
    assert engine.group_commit_eval(grp, flat["commitments"], pos) == engine.commit_eval(flat["commitments"], pos)
    args = (flat["commitments"], flat["positions"], flat["publickeys"], flat["shares"], flat["responses"], flat["challenge"])
    a = engine.group_verify_distribution(grp, *args, dump=True)
    b = engine.verify_distribution(*args, dump=True)
    assert a == b and a["verdict"] is True


def _check_protocol(engine, q, n, t, seed):
    g, privs, pks, box = H.make_instance(q, n, t, seed)
    grp = ModpGroup(q)
    flat = O.box_to_flat(g, box)
    args = [flat["commitments"], flat["positions"], flat["publickeys"], flat["shares"], flat["responses"], flat["challenge"]]
    trace = {}
    ok = O.verify_distribution_shares(g, box, trace)
    res = engine.group_verify_distribution(grp, *args, dump=True)
    assert res["verdict"] is ok is True and res["digest"] == trace["digest"]
    assert split(res["X"]) == trace["X"] and split(res["a1"]) == trace["a1"] and split(res["a2"]) == trace["a2"]
    # a changed Y_i, r_i or challenge is rejected
    for field, k in (("shares", 3), ("responses", 4)):
        bad = bytearray(args[k])
        bad[-1] ^= 1
        a2 = list(args)
        a2[k] = bytes(bad)
        assert engine.group_verify_distribution(grp, *a2)["verdict"] is False, field
    a2 = list(args)
    a2[5] = enc(box["challenge"] + 1)
    assert engine.group_verify_distribution(grp, *a2)["verdict"] is False
    # verify_share of every participant, tampered rows included
    rng = random.Random(seed + 1)
    sbs = [O.extract_secret_share(g, box, k, H.keygen(g, rng)) for k in privs]
    keys = [g.element_to_bytes(p) for p in pks]
    S = [s["share"] for s in sbs]
    C = [s["challenge"] for s in sbs]
    R = [s["response"] for s in sbs]
    if len(S) > 1:
        R[1] = (R[1] + 1) % (q - 1)
        C[0] = (C[0] + 1)
    want = []
    for i, pk in enumerate(pks):
        sb = dict(sbs[i], challenge=C[i], response=R[i])
        want.append(1 if O.verify_share(g, sb, box, pk) else 0)
    got = engine.group_verify_shares(grp, cat(pks), cat(S), cat([box["shares"][k] for k in keys]), cat(C), cat(R))
    assert list(got) == want
    return g, grp, box


@pytest.mark.parametrize("bits,n,t", [(64, 12, 3), (256, 10, 4), (768, 6, 3), (1024, 5, 2), (1536, 4, 2)])
def test_protocol_against_the_oracle(engine, bits, n, t):
    q = H.rfc_prime(bits) if bits in H.RFC_C else H.small_safe_primes()[bits]
    _check_protocol(engine, q, n, t, seed=bits)


def test_protocol_edge_shapes(engine):
    q = H.small_safe_primes()[256]
    g, grp, box = _check_protocol(engine, q, 5, 1, seed=5)          # t = 1
    res = engine.group_verify_distribution(grp, b"", [], b"", b"", b"", enc(box["challenge"]))   # n = 0: empty transcript
    import hashlib
    d = hashlib.sha256(b"").digest()
    assert res["digest"] == d
    assert res["verdict"] is (int.from_bytes(hashlib.sha256(d).digest(), "big") % g.g == box["challenge"])


def test_position_multiple_of_order_and_zero_commitment(engine):
    """i' = i mod (q-1): a position that is a multiple of q - 1 with a commitment = 0 mod q gives C_0 (reference order), and a
    position past q - 1 the reduced exponent's value"""
    for q in (H.small_safe_primes()[40], H.small_safe_primes()[64]):
        g = H.RtOracleGroup(q)
        grp = ModpGroup(q)
        cms = [7, 0, q, 12345 % q]
        pos = [0, 1, 2, q - 1, 3, (q - 1) * 2 + 5]
        pos = [p for p in pos if p < (1 << 63)]
        want = [O.commitment_eval(g, cms, p) for p in pos]
        assert split(engine.group_commit_eval(grp, cat(cms), pos)) == want, q.bit_length()


def test_four_threads_on_one_context(engine):
    rng = random.Random(4)
    groups = [ModpGroup(H.rfc_prime(768)), ModpGroup(H.small_safe_primes()[256])]
    jobs = []
    for k in range(8):
        grp = groups[k % 2]
        B = [rng.randrange(1 << 2048) for _ in range(64)]
        E = [rng.randrange(1 << 512) for _ in range(64)]
        jobs.append((grp, B, E, [pow(b, e, grp.q) for b, e in zip(B, E)]))
    errors = []

    def work(my):
        try:
            for grp, B, E, want in my:
                assert split(engine.group_batch_exp(grp, cat(B), cat(E))) == want
                assert split(engine.group_batch_mul(grp, cat(B), cat(E))) == [b * e % grp.q for b, e in zip(B, E)]
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(jobs[i::4],)) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
