"""Run-time MODP groups, the rest of the protocol on the GPU: two powers of one base (both sides of the crossover), the dealer
(group_deal / group_distribute), extract_secret_share and reconstruct against the oracle over RtOracleGroup(q) at 40 .. 2048
bits, and group 14 through the run-time path against the group-14 entry points."""
import hashlib
import math
import random
import threading

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
from helpers import make_modp_instance
from mpvss_rs_amd import ModpGroup, capi

pytestmark = pytest.mark.gpu

EB = 256
TOP = (1 << 2048) - 1


def _twin_min_shares(grp):
    """the library's crossover for the group's width (mpvss_modp_group_twin_min_shares): batches from this size take
    k_rt_twin_exp, smaller ones the two exponent sets"""
    m = grp.twin_min_shares
    # both sides must be reachable in one chunk and the edge rows of _twin_inputs must fit: true of the default build only
    assert 24 < m <= 65536, (f"twin_min_shares = {m}: the crossover tests need the default build's constant, not a library "
                             "with the dispatch pinned to one path (make twin-ab) -- this is not an arithmetic failure")
    return m


def enc(v):
    return (v % (1 << 2048)).to_bytes(EB, "big")


def cat(vals):
    return b"".join(enc(v) for v in vals)


def split(b):
    return [int.from_bytes(b[i:i + EB], "big") for i in range(0, len(b), EB)]


def _moduli():
    """the MODULI list of tests/test_gpu_modp_rt.py, rebuilt from modp_rt_helpers"""
    rng = random.Random(11)
    out = []
    for bits in (578, 579, 1042, 1043, 2047, 2048):
        q = H.random_odd_modulus(bits, rng)
        while q % (1 << 29) == (1 << 29) - 1:
            q = H.random_odd_modulus(bits, rng)
        out.append(q)
    for k in (64, 580, 1044, 2048):
        out.append(2 ** k - 1)
        out.append(2 ** (k - 1) + 1)
    out += [H.rfc_prime(1024), H.small_safe_primes()[64], 5, 23]
    return out


MODULI = _moduli()


def _prime(bits):
    return H.rfc_prime(bits) if bits in H.RFC_C else H.small_safe_primes()[bits]


@pytest.mark.parametrize("q", MODULI, ids=[f"{q.bit_length()}b" for q in MODULI])
def test_twin_exp_matches_python(engine, q):
    grp = ModpGroup(q)
    rng = random.Random(q & 0xFFFF)
    bases = [b for b in (0, 1, q - 1, q, q + 1) if b <= TOP] + [TOP]
    exps = [0, 1, max(q - 2, 0), TOP]
    cases = [(b, e1, e2) for b in bases for e1 in exps for e2 in exps]
    for n in (1, 15, 16, 17, 33):
        for start in range(0, len(cases), n):
            chunk = cases[start:start + n]
            while len(chunk) < n:
                chunk.append((rng.randrange(1 << 2048), rng.randrange(1 << rng.choice((1, 64, q.bit_length(), 2048))),
                              rng.randrange(1 << rng.choice((1, 64, q.bit_length(), 2048)))))
            B, E1, E2 = zip(*chunk)
            o1, o2 = engine.group_batch_twin_exp(grp, cat(B), cat(E1), cat(E2))
            assert split(o1) == [pow(b, e, q) for b, e in zip(B, E1)], (q.bit_length(), n, start)
            assert split(o2) == [pow(b, e, q) for b, e in zip(B, E2)], (q.bit_length(), n, start)


def _twin_inputs(q, n, rng, ebits):
    edge_b = [0, 1, q - 1, q, q + 1, TOP]
    edge_e = [0, 1, max(q - 2, 0), TOP]
    B = [edge_b[i % 6] if i < 24 else rng.randrange(1 << 2048) for i in range(n)]
    E1 = [edge_e[i % 4] if i < 24 else rng.randrange(1 << rng.choice(ebits)) for i in range(n)]
    E2 = [edge_e[(i // 4) % 4] if i < 24 else rng.randrange(1 << rng.choice(ebits)) for i in range(n)]
    return B, E1, E2


@pytest.mark.parametrize("bits", [64, 256])
def test_both_sides_of_the_crossover_small_widths(engine, bits):
    q = H.small_safe_primes()[bits]
    grp = ModpGroup(q)
    rng = random.Random(bits)
    m = _twin_min_shares(grp)
    for n in (m - 3, m, m + 5):
        B, E1, E2 = _twin_inputs(q, n, rng, (8, bits, bits, 2048))
        o1, o2 = engine.group_batch_twin_exp(grp, cat(B), cat(E1), cat(E2))
        assert split(o1) == [pow(b, e, q) for b, e in zip(B, E1)], n
        assert split(o2) == [pow(b, e, q) for b, e in zip(B, E2)], n


def test_both_sides_of_the_crossover_2048(engine):
    q = H.rfc_prime(2048)
    grp = ModpGroup(q)
    rng = random.Random(2048)
    for n in (_twin_min_shares(grp) - 3, _twin_min_shares(grp) + 5):
        B, E1, E2 = _twin_inputs(q, n, rng, (8, 300, 2048))
        o1, o2 = engine.group_batch_twin_exp(grp, cat(B), cat(E1), cat(E2))
        g1, g2 = split(o1), split(o2)
        idx = sorted(set(list(range(0, n, max(1, n // 200))) + list(range(24)) + [n - 1]))
        assert [g1[i] for i in idx] == [pow(B[i], E1[i], q) for i in idx], n
        assert [g2[i] for i in idx] == [pow(B[i], E2[i], q) for i in idx], n
    # the two paths give identical bytes: the same rows below and above the constant
    n = _twin_min_shares(grp)
    B, E1, E2 = _twin_inputs(q, n, rng, (2048,))
    big = engine.group_batch_twin_exp(grp, cat(B), cat(E1), cat(E2))
    m = 37
    small = engine.group_batch_twin_exp(grp, cat(B[:m]), cat(E1[:m]), cat(E2[:m]))
    assert big[0][: m * EB] == small[0] and big[1][: m * EB] == small[1]


def _instance(q, n, t, seed):
    """a box of the oracle's own dealer over the group of q, with the randomness kept (helpers.make_instance drops it)"""
    g = H.RtOracleGroup(q)
    rng = random.Random(seed)
    privs, pks, seen = [], [], set()
    while len(pks) < n:
        k = H.keygen(g, rng)
        pk = g.generate_public_key(k)
        if pk not in seen:                 # the box maps shares by the key's bytes
            seen.add(pk)
            privs.append(k)
            pks.append(pk)
    coeffs = [rng.randrange(g.q - 1) for _ in range(t)]
    coeffs[0] = coeffs[0] or 1
    ws = [H.keygen(g, rng) for _ in range(n)]
    box = O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)
    return g, privs, pks, coeffs, ws, box


def _check_deal(engine, g, grp, pks, coeffs, ws, box):
    n = len(pks)
    keys = [g.element_to_bytes(p) for p in pks]
    positions = list(range(1, n + 1))
    res = engine.group_deal(grp, cat(coeffs), positions, cat(pks), cat(ws))
    assert split(res["X"]) == box["_X"] and split(res["a1"]) == box["_a1"] and split(res["a2"]) == box["_a2"]
    assert split(res["Y"]) == [box["shares"][k] for k in keys]
    assert res["digest"] == box["_digest"]
    assert split(res["challenge"]) == [box["challenge"]]
    assert split(res["responses"]) == [box["responses"][k] for k in keys]
    flat = O.box_to_flat(g, box)
    v = engine.group_verify_distribution(grp, flat["commitments"], positions, cat(pks), res["Y"], res["responses"], res["challenge"])
    assert v["verdict"] is True and v["digest"] == res["digest"]
    P = [O.poly_get_value(coeffs, i) % (g.q - 1) for i in positions]
    d = engine.group_distribute(grp, flat["commitments"], positions, cat(pks), cat(P), cat(ws))
    assert all(d[k] == res[k] for k in ("X", "Y", "a1", "a2", "digest"))
    return res


def _check_extract(engine, g, grp, privs, pks, box, seed):
    rng = random.Random(seed)
    keys = [g.element_to_bytes(p) for p in pks]
    Y = [box["shares"][k] for k in keys]
    ws = [H.keygen(g, rng) for _ in privs]
    sbs = [O.extract_secret_share(g, box, k, w) for k, w in zip(privs, ws)]
    assert all(sb is not None for sb in sbs)
    xinv = [O.mod_inverse(k, g.q - 1) for k in privs]
    S, C = engine.group_extract_shares(grp, cat(pks), cat(Y), cat(xinv), cat(ws))
    assert split(S) == [sb["share"] for sb in sbs] and split(C) == [sb["challenge"] for sb in sbs]
    R = capi.group_dleq_responses(grp, cat(ws), cat(privs), C)
    assert split(R) == [sb["response"] for sb in sbs]
    assert list(engine.group_verify_shares(grp, cat(pks), S, cat(Y), C, R)) == [1] * len(pks)
    return sbs


def _secret_from(g, box, mask):
    return int.from_bytes(mask, "big") ^ box["U"]


def _picks(n, t):
    """all n shares; exactly t shares at evenly spread, non-contiguous positions (negative Lagrange factors occur)"""
    spread = sorted({round(i * (n - 1) / (t - 1)) for i in range(t)}) if t >= 2 else [n // 2]
    assert len(spread) == t
    return [list(range(n)), spread]


def _oracle_recovers(g, privs, pks, box, t):
    sbs = [O.extract_secret_share(g, box, k, 1) for k in privs]
    return all(O.reconstruct(g, [sbs[i] for i in pick], box) == 0x1234 for pick in _picks(len(pks), t))


def _recoverable_instance(q, n, t, seed, recovers=True):
    """The reference reduces the Lagrange exponents mod (q-1)/2 (participant.rs:540-548) while G = 2 has order q - 1 whenever 2
    is a non-residue (q = 3 mod 8: the 64-bit fixture prime): its own reconstruct then recovers G^s only up to the sign, by the
    parity of the quotient.  The round trip needs a box the REFERENCE recovers: the first seed in a fixed sequence where it does
    (the first one for every q = 7 mod 8, the RFC primes included).  recovers=False: the first box it does not recover."""
    for attempt in range(64):
        inst = _instance(q, n, t, seed + 1000 * attempt)
        g, privs, pks, coeffs, ws, box = inst
        if _oracle_recovers(g, privs, pks, box, t) == recovers:
            assert attempt == 0 or q % 8 == 3
            return inst
    raise AssertionError("no such box in 64 seeds")


def _check_reconstruct(engine, g, grp, sbs, box, pks, t, secret=0x1234):
    keys = [g.element_to_bytes(p) for p in pks]
    pos = [box["positions"][k] for k in keys]
    for pick in _picks(len(pks), t):
        sub = [sbs[i] for i in pick]
        want = O.reconstruct(g, sub, box)
        assert want is not None and (secret is None or want == secret)
        gs, mask = engine.group_reconstruct(grp, [pos[i] for i in pick], cat([sbs[i]["share"] for i in pick]))
        assert _secret_from(g, box, mask) == want
        assert int.from_bytes(mask, "big") == g.secret_mask(int.from_bytes(gs, "big"))
        # an order the oracle does not see (it sorts): the same product
        rev = list(reversed(pick))
        assert engine.group_reconstruct(grp, [pos[i] for i in rev], cat([sbs[i]["share"] for i in rev])) == (gs, mask)


@pytest.mark.parametrize("bits,n,t", [(64, 12, 3), (256, 10, 4), (768, 6, 3), (1024, 5, 2), (1536, 4, 2), (2048, 4, 2), (256, 5, 1)])
def test_deal_extract_reconstruct_against_the_oracle(engine, bits, n, t):
    q = _prime(bits)
    grp = ModpGroup(q)
    g, privs, pks, coeffs, ws, box = _recoverable_instance(q, n, t, seed=bits + t)
    _check_deal(engine, g, grp, pks, coeffs, ws, box)
    sbs = _check_extract(engine, g, grp, privs, pks, box, seed=bits)
    _check_reconstruct(engine, g, grp, sbs, box, pks, t)
    if t == 1:        # m = 1 with t = 1
        k0 = g.element_to_bytes(pks[2])
        gs, mask = engine.group_reconstruct(grp, [box["positions"][k0]], enc(sbs[2]["share"]))
        assert _secret_from(g, box, mask) == O.reconstruct(g, [sbs[2]], box) == 0x1234


def test_reconstruct_follows_the_reference_where_it_loses_the_sign(engine):
    """q = 3 mod 8: a box whose secret the reference's own reconstruct does not recover -- the engine returns the same value"""
    q = H.small_safe_primes()[64]
    assert q % 8 == 3
    grp = ModpGroup(q)
    g, privs, pks, coeffs, ws, box = _recoverable_instance(q, 12, 3, seed=64, recovers=False)
    sbs = [O.extract_secret_share(g, box, k, 1) for k in privs]
    _check_reconstruct(engine, g, grp, sbs, box, pks, 3, secret=None)


def test_negative_lagrange_factors_do_occur():
    """the t-share case above must exercise the inverted factors"""
    num, den = O.lagrange_coefficient(5, [1, 5, 12])
    assert num * den < 0


def test_group14_through_the_runtime_path_is_byte_identical(engine):
    g, privs, pks, coeffs, ws, box = make_modp_instance(9, 4, seed=77, secret=0x1234)
    grp = ModpGroup(g.q)
    positions = list(range(1, 10))
    a = engine.group_deal(grp, cat(coeffs), positions, cat(pks), cat(ws))
    b = engine.deal(cat(coeffs), positions, cat(pks), cat(ws))
    assert a == b
    keys = [g.element_to_bytes(p) for p in pks]
    Y = cat([box["shares"][k] for k in keys])
    rng = random.Random(5)
    w2 = [H.keygen(g, rng) for _ in privs]
    xinv = [O.mod_inverse(k, g.q - 1) for k in privs]
    ea = engine.group_extract_shares(grp, cat(pks), Y, cat(xinv), cat(w2))
    eb = engine.extract_shares(cat(pks), Y, cat(xinv), cat(w2))
    assert ea == eb
    for pick in (list(range(9)), [0, 3, 4, 8]):
        pos = [positions[i] for i in pick]
        S = b"".join(ea[0][i * EB:(i + 1) * EB] for i in pick)
        assert engine.group_reconstruct(grp, pos, S) == engine.reconstruct(pos, S)


def test_extract_with_encrypted_shares_that_are_zero_mod_q(engine):
    for bits in (64, 1024):
        q = _prime(bits)
        grp = ModpGroup(q)
        g, privs, pks, coeffs, ws, box = _instance(q, 6, 3, seed=bits)
        keys = [g.element_to_bytes(p) for p in pks]
        box = dict(box, shares=dict(box["shares"]))
        box["shares"][keys[1]] = 0
        box["shares"][keys[4]] = q
        rng = random.Random(9)
        w2 = [H.keygen(g, rng) for _ in privs]
        sbs = [O.extract_secret_share(g, box, k, w) for k, w in zip(privs, w2)]
        assert sbs[1]["share"] == 0 and sbs[4]["share"] == 0
        xinv = [O.mod_inverse(k, q - 1) for k in privs]
        S, C = engine.group_extract_shares(grp, cat(pks), cat([box["shares"][k] for k in keys]), cat(xinv), cat(w2))
        assert split(S) == [sb["share"] for sb in sbs] and split(C) == [sb["challenge"] for sb in sbs]


def test_lagrange_denominators_are_invertible_for_the_fixture_primes():
    """with positions <= 12 every Lagrange denominator is a product of integers below 12 < (q-1)/2 prime, so the oracle's
    reconstruct never returns None on these inputs (checked on the CPU, part of the 40-bit round trip's premise)"""
    for bits, q in H.small_safe_primes().items():
        sub = (q - 1) // 2
        assert H.miller_rabin(q) and H.miller_rabin(sub), bits
        assert all(math.gcd(d, sub) == 1 for d in range(1, 13))


def test_round_trip_at_40_bits(engine):
    q = H.small_safe_primes()[40]
    grp = ModpGroup(q)
    g, privs, pks, coeffs, ws, box = _recoverable_instance(q, 12, 5, seed=40)
    res = _check_deal(engine, g, grp, pks, coeffs, ws, box)
    assert res["Y"] == O.box_to_flat(g, box)["shares"]
    sbs = _check_extract(engine, g, grp, privs, pks, box, seed=41)
    _check_reconstruct(engine, g, grp, sbs, box, pks, 5)


def test_errors_and_the_empty_box(engine):
    q = H.small_safe_primes()[256]
    grp = ModpGroup(q)
    g, privs, pks, coeffs, ws, box = _instance(q, 4, 2, seed=1)
    with pytest.raises(capi.EngineError, match="rc=-1"):
        engine.group_deal(grp, cat(coeffs + [1, 2, 3]), [1, 2, 3, 4], cat(pks), cat(ws))          # t > n
    with pytest.raises(capi.EngineError, match="rc=-1"):
        engine.group_deal(grp, b"", [1, 2, 3, 4], cat(pks), cat(ws))                               # t == 0, n > 0
    with pytest.raises(capi.EngineError, match="rc=-1"):
        engine.group_deal(grp, cat(coeffs), [1, -2, 3, 4], cat(pks), cat(ws))                      # negative position
    res = engine.group_deal(grp, b"", [], b"", b"")                                                # n == 0
    d = hashlib.sha256(b"").digest()
    assert res["digest"] == d and split(res["challenge"]) == [g.hash_to_scalar(d)]
    shares = cat([3, 4, 5])
    for pos in ([1, 1, 2], [0, 1, 2]):
        with pytest.raises(capi.EngineError, match="rc=-1"):
            engine.group_reconstruct(grp, pos, shares)
    with pytest.raises(capi.EngineError, match="rc=-1"):
        engine.group_reconstruct(grp, [], b"")                                                     # m == 0
    # a share that is 0 mod q under a negative Lagrange factor has no inverse
    with pytest.raises(capi.EngineError, match="rc=-1"):
        engine.group_reconstruct(grp, [1, 5, 12], cat([3, q, 5]))
    # the engine still works after the refusals
    assert split(engine.group_batch_twin_exp(grp, enc(3), enc(5), enc(7))[0]) == [243]


def test_four_threads_on_one_context(engine):
    jobs = []
    for k, bits in enumerate((768, 256, 768, 256, 768, 256, 768, 256)):
        q = _prime(bits)
        grp = ModpGroup(q)
        g, privs, pks, coeffs, ws, box = _instance(q, 5, 2, seed=100 + k)
        jobs.append((g, grp, privs, pks, coeffs, ws, box))

    def run(job, k):
        g, grp, privs, pks, coeffs, ws, box = job
        keys = [g.element_to_bytes(p) for p in pks]
        deal = engine.group_deal(grp, cat(coeffs), list(range(1, len(pks) + 1)), cat(pks), cat(ws))
        xinv = [O.mod_inverse(x, g.q - 1) for x in privs]
        ext = engine.group_extract_shares(grp, cat(pks), cat([box["shares"][x] for x in keys]), cat(xinv), cat(ws))
        tw = engine.group_batch_twin_exp(grp, cat(pks), cat(coeffs * 3)[: len(pks) * EB], cat(ws))
        return deal, ext, tw

    want = [run(j, k) for k, j in enumerate(jobs)]
    for j, w in zip(jobs, want):
        g, grp, privs, pks, coeffs, ws, box = j
        assert split(w[0]["Y"]) == [box["shares"][g.element_to_bytes(p)] for p in pks]
    got = [None] * len(jobs)
    errors = []

    def work(idx):
        try:
            for k in idx:
                got[k] = run(jobs[k], k)
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(list(range(i, len(jobs), 4)),)) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    assert got == want
