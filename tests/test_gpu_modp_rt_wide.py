"""Wide run-time MODP groups on the GPU (mpvss_modp_group_create_wide: 384-byte elements, 27 limbs per lane, moduli of 2049 ..
3072 bits): exp / mul / twin / fixed base against Python's pow at the share counts around one workgroup's 16 numbers, both
sides of the comb and twin launch decisions, the whole protocol on RFC 3526 group 15 against the oracle over
RtOracleGroup, and a 256-byte handle next to a wide one in the same process."""
import random

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
from mpvss_rs_amd import Engine, ModpGroup, capi

pytestmark = pytest.mark.gpu

EB, TOP = WH.EB, WH.TOP
cat, split, be = WH.cat, WH.split, WH.be
SIZES = (1, 15, 16, 17, 33)          # one workgroup's 16 numbers, one less, one more, and a ragged tail
MODULI = {"group15": WH.group15, "2^3072-1": lambda: TOP, "odd2049": WH.odd_2049}


@pytest.fixture(scope="module", params=sorted(MODULI))
def wide(request):
    q = MODULI[request.param]()
    grp = ModpGroup(q, elem_bytes=EB)
    assert (grp.elem_bytes, grp.limbs_per_lane) == (384, 27)
    yield q, grp
    grp.close()


@pytest.fixture(scope="module")
def grp15():
    grp = ModpGroup(WH.group15(), elem_bytes=EB)
    yield grp
    grp.close()


def _bases(q):
    """0, 1, q - 1, q, q + 1, 2^3072 - 1 (q + 1 has no 384-byte encoding when q = 2^3072 - 1)"""
    return [b for b in (0, 1, q - 1, q, q + 1) if b <= TOP] + [TOP]


def _exps(q, rng):
    """0, 1, q - 1, 2^3072 - 1, only the top nibble, only bit 2048 (the first bit a 256-byte edge would lose), random"""
    return [0, 1, q - 1, TOP, 0xF << 3068, 1 << 2048, rng.getrandbits(3072), rng.getrandbits(2049)]


def _batches(rows, rng, fill):
    """rows cut into batches of SIZES, in turn, the last one filled up with fill(rng)"""
    out, i, k = [], 0, 0
    while i < len(rows):
        n = SIZES[k % len(SIZES)]
        chunk = rows[i:i + n]
        while len(chunk) < n:
            chunk.append(fill(rng))
        out.append(chunk)
        i += n
        k += 1
    assert {len(c) for c in out} == set(SIZES)
    return out


def test_batch_exp_matches_pow(engine, wide):
    q, grp = wide
    rng = random.Random(1)
    rows = [(b, e) for b in _bases(q) for e in _exps(q, rng)] + [(rng.getrandbits(3072), rng.getrandbits(3072)) for _ in range(40)]
    for chunk in _batches(rows, rng, lambda r: (r.getrandbits(3072), r.getrandbits(r.choice((1, 64, 2049, 3072))))):
        B, E = zip(*chunk)
        out = engine.group_batch_exp(grp, cat(B), cat(E))
        assert len(out) == len(B) * EB
        assert split(out) == [pow(b, e, q) for b, e in zip(B, E)], len(B)


def test_mixed_lengths_within_one_wave(engine, wide):
    """the wave's highest bit comes from one lane only: every other number of the wave idles through its windows"""
    q, grp = wide
    rng = random.Random(2)
    for long_row, long_e in ((5, TOP), (0, 1 << 3071), (15, 1 << 2048)):
        E = [rng.getrandbits(rng.choice((1, 8, 64))) for _ in range(16)]
        E[long_row] = long_e
        E[(long_row + 3) % 16] = 0
        B = [rng.getrandbits(3072) for _ in range(16)]
        assert split(engine.group_batch_exp(grp, cat(B), cat(E))) == [pow(b, e, q) for b, e in zip(B, E)]
        o1, o2 = engine.group_batch_twin_exp(grp, cat(B), cat(E), cat(E[::-1]))
        assert split(o1) == [pow(b, e, q) for b, e in zip(B, E)] and split(o2) == [pow(b, e, q) for b, e in zip(B, E[::-1])]
        assert split(engine.group_batch_exp_fixed_base(grp, be(B[0]), cat(E))) == [pow(B[0], e, q) for e in E]


def test_batch_mul_matches_python(engine, wide):
    q, grp = wide
    rng = random.Random(3)
    vals = _bases(q) + [q - 2, 2, 1 << 2048]
    rows = [(a, b) for a in vals for b in vals]
    for chunk in _batches(rows, rng, lambda r: (r.getrandbits(3072), r.getrandbits(3072))):
        A, B = zip(*chunk)
        assert split(engine.group_batch_mul(grp, cat(A), cat(B))) == [a * b % q for a, b in zip(A, B)], len(A)


def test_batch_twin_exp_matches_pow(engine, wide):
    q, grp = wide
    rng = random.Random(4)
    ex = _exps(q, rng)
    rows = [(b, ex[i % len(ex)], ex[(i // 2 + 3 * k) % len(ex)]) for k, b in enumerate(_bases(q)) for i in range(len(ex))]
    rows += [(rng.getrandbits(3072), rng.getrandbits(3072), rng.getrandbits(2049)) for _ in range(16)]
    for chunk in _batches(rows, rng, lambda r: (r.getrandbits(3072), r.getrandbits(3072), r.getrandbits(64))):
        B, E1, E2 = zip(*chunk)
        o1, o2 = engine.group_batch_twin_exp(grp, cat(B), cat(E1), cat(E2))
        assert split(o1) == [pow(b, e, q) for b, e in zip(B, E1)], len(B)
        assert split(o2) == [pow(b, e, q) for b, e in zip(B, E2)], len(B)


def test_batch_exp_fixed_base_matches_pow(engine, wide):
    """below comb_min_shares on a context that has no comb of these bases: the 16-entry table path"""
    q, grp = wide
    rng = random.Random(5)
    assert max(SIZES) < grp.comb_min_shares
    bases = _bases(q) + [rng.getrandbits(3072)]
    for k, base in enumerate(bases):
        n = SIZES[k % len(SIZES)]
        E = (_exps(q, rng) + [rng.getrandbits(rng.choice((8, 3072))) for _ in range(n)])[k:][:n]
        out = engine.group_batch_exp_fixed_base(grp, be(base), cat(E))
        assert split(out) == [pow(base, e, q) for e in E], (k, n)


def test_fixed_base_on_both_sides_of_the_launch_decision():
    """two wide groups and one 256-byte group on ONE context of their own: without prepare a small call takes the 16-entry table
    (no build, no hit); after prepare the comb (hit), same bytes; the cache keeps (q, base) of the three groups apart"""
    eng = Engine(0)
    rng = random.Random(6)
    qa, qb, qc = WH.group15(), WH.odd_2049(), H.rfc_prime(2048)
    ga, gb, gc = ModpGroup(qa, elem_bytes=EB), ModpGroup(qb, elem_bytes=EB), ModpGroup(qc)
    try:
        n = 33
        assert n < ga.comb_min_shares and n < gc.comb_min_shares
        Ew = [0, 1, qa - 1, TOP, 0xF << 3068, 1 << 2048] + [rng.getrandbits(3072) for _ in range(n - 6)]
        En = [e % (1 << 2048) for e in Ew]
        call = {
            "a": lambda: eng.group_batch_exp_fixed_base(ga, be(4), cat(Ew)),
            "b": lambda: eng.group_batch_exp_fixed_base(gb, be(4), cat(Ew)),
            "c": lambda: eng.group_batch_exp_fixed_base(gc, be(4, 256), cat(En, 256)),
        }
        want = {"a": cat([pow(4, e, qa) for e in Ew]), "b": cat([pow(4, e, qb) for e in Ew]), "c": cat([pow(4, e, qc) for e in En], 256)}
        table = {k: f() for k, f in call.items()}
        assert table == want
        assert eng.group_comb_stats() == {"builds": 0, "hits": 0, "evictions": 0}
        eng.group_prepare(ga)
        eng.group_prepare(gb)
        assert eng.group_comb_stats() == {"builds": 4, "hits": 0, "evictions": 0}        # g = 4 and G = 2 of each group
        assert call["a"]() == want["a"] and call["b"]() == want["b"]
        assert eng.group_comb_stats() == {"builds": 4, "hits": 2, "evictions": 0}
        assert call["c"]() == want["c"]                                                   # same base bytes' value, other q and size
        assert eng.group_comb_stats() == {"builds": 4, "hits": 2, "evictions": 0}
        eng.group_prepare(gc)                                                             # 4 slots: the two oldest go
        assert eng.group_comb_stats() == {"builds": 6, "hits": 2, "evictions": 2}
        assert call["c"]() == want["c"] and call["a"]() == want["a"] and call["b"]() == want["b"]
        assert eng.group_comb_stats()["hits"] >= 3
        # G = 2 through the comb as well (generate_public_key)
        eng.group_prepare(ga)
        assert eng.group_batch_exp_fixed_base(ga, be(2), cat(Ew)) == cat([pow(2, e, qa) for e in Ew])
    finally:
        for g in (ga, gb, gc):
            g.close()
        eng.close()


def test_twin_on_both_sides_of_its_crossover(engine, grp15):
    """k_rt_twin_exp at twin_min_shares shares, once; the same rows through the two exponent sets in calls below the
    crossover: equal bytes everywhere, and equal to pow on a sample of 64 positions"""
    q = WH.group15()
    m = grp15.twin_min_shares
    assert 33 < m <= 32768 and m % 2 == 0, f"twin_min_shares = {m}: this test needs the default build's constant"
    rng = random.Random(7)
    edge_b, edge_e = _bases(q), [0, 1, q - 1, TOP, 0xF << 3068, 1 << 2048]
    assert len(edge_b) == 6
    B = [edge_b[i % 6] if i < 36 else rng.getrandbits(3072) for i in range(m)]
    E1 = [edge_e[i % 6] if i < 36 else rng.getrandbits(rng.choice((8, 300, 3072))) for i in range(m)]
    E2 = [edge_e[(i // 6) % 6] if i < 36 else rng.getrandbits(rng.choice((8, 2049, 3072))) for i in range(m)]
    cb, c1, c2 = cat(B), cat(E1), cat(E2)
    big = engine.group_batch_twin_exp(grp15, cb, c1, c2)
    small = engine.group_batch_twin_exp(grp15, cb[:33 * EB], c1[:33 * EB], c2[:33 * EB])
    assert big[0][:33 * EB] == small[0] and big[1][:33 * EB] == small[1]
    half = m // 2 * EB
    lo = engine.group_batch_twin_exp(grp15, cb[:half], c1[:half], c2[:half])
    hi = engine.group_batch_twin_exp(grp15, cb[half:], c1[half:], c2[half:])
    assert big[0] == lo[0] + hi[0] and big[1] == lo[1] + hi[1]
    g1, g2 = split(big[0]), split(big[1])
    idx = sorted(set(list(range(36)) + [m - 1] + [rng.randrange(m) for _ in range(27)]))[:64]
    assert [g1[i] for i in idx] == [pow(B[i], E1[i], q) for i in idx]
    assert [g2[i] for i in idx] == [pow(B[i], E2[i], q) for i in idx]


# ---- the protocol on group 15 ----------------------------------------------------------------------------------------
def _instance(q, n, t, seed):
    g = H.RtOracleGroup(q)
    rng = random.Random(seed)
    privs = [H.keygen(g, rng) for _ in range(n)]
    pks = [g.generate_public_key(k) for k in privs]
    assert len(set(pks)) == n
    coeffs = [rng.randrange(1, g.q - 1) for _ in range(t)]
    ws = [H.keygen(g, rng) for _ in range(n)]
    box = O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)
    return g, privs, pks, coeffs, ws, box


def _flip(buf, row, byte=EB - 1):
    b = bytearray(buf)
    b[row * EB + byte] ^= 1
    return bytes(b)


@pytest.mark.parametrize("n,t", [(5, 3), (33, 17), (3, 1)])
def test_protocol_on_group15_against_the_oracle(engine, grp15, n, t):
    q = WH.group15()
    g, privs, pks, coeffs, ws, box = _instance(q, n, t, seed=100 * n + t)
    keys = [g.element_to_bytes(p) for p in pks]
    positions = list(range(1, n + 1))
    assert [box["positions"][k] for k in keys] == positions
    # deal: every byte of the box and of the proofs
    res = engine.group_deal(grp15, cat(coeffs), positions, cat(pks), cat(ws))
    assert split(res["X"]) == box["_X"] and split(res["a1"]) == box["_a1"] and split(res["a2"]) == box["_a2"]
    assert split(res["Y"]) == [box["shares"][k] for k in keys]
    assert res["digest"] == box["_digest"]
    assert split(res["challenge"]) == [box["challenge"]]
    assert split(res["responses"]) == [box["responses"][k] for k in keys]
    C = cat(box["commitments"])
    assert split(engine.group_batch_exp_fixed_base(grp15, be(4), cat(coeffs))) == box["commitments"]
    # verify_distribution, and one tampered Y_i / response
    v = engine.group_verify_distribution(grp15, C, positions, cat(pks), res["Y"], res["responses"], res["challenge"], dump=True)
    assert v["verdict"] is True and v["digest"] == res["digest"]
    assert (v["X"], v["a1"], v["a2"]) == (res["X"], res["a1"], res["a2"])
    for bad_y, bad_r in ((_flip(res["Y"], n // 2), res["responses"]), (res["Y"], _flip(res["responses"], n - 1, 17))):
        assert engine.group_verify_distribution(grp15, C, positions, cat(pks), bad_y, bad_r, res["challenge"])["verdict"] is False
    # distribute with the commitments (Horner in the exponent over t of them)
    P = [O.poly_get_value(coeffs, i) % (q - 1) for i in positions]
    d = engine.group_distribute(grp15, C, positions, cat(pks), cat(P), cat(ws))
    assert all(d[k] == res[k] for k in ("X", "Y", "a1", "a2", "digest"))
    # extract_secret_share and its proofs
    rng = random.Random(n)
    w2 = [H.keygen(g, rng) for _ in privs]
    sbs = [O.extract_secret_share(g, box, k, w) for k, w in zip(privs, w2)]
    assert all(sb is not None for sb in sbs)
    xinv = [O.mod_inverse(k, q - 1) for k in privs]
    S, Cs = engine.group_extract_shares(grp15, cat(pks), res["Y"], cat(xinv), cat(w2))
    assert split(S) == [sb["share"] for sb in sbs] and split(Cs) == [sb["challenge"] for sb in sbs]
    R = capi.group_dleq_responses(grp15, cat(w2), cat(privs), Cs)
    assert split(R) == [sb["response"] for sb in sbs]
    assert list(engine.group_verify_shares(grp15, cat(pks), S, res["Y"], Cs, R)) == [1] * n
    bad = n // 3
    assert list(engine.group_verify_shares(grp15, cat(pks), _flip(S, bad), res["Y"], Cs, R)) == [int(i != bad) for i in range(n)]
    assert list(engine.group_verify_shares(grp15, cat(pks), S, res["Y"], Cs, _flip(R, n - 1, 200))) == [1] * (n - 1) + [0]
    # reconstruct from all n shares and from exactly t spread ones
    spread = sorted({round(i * (n - 1) / (t - 1)) for i in range(t)}) if t >= 2 else [n // 2]
    for pick in (list(range(n)), spread):
        want = O.reconstruct(g, [sbs[i] for i in pick], box)
        assert want == 0x1234
        gs, mask = engine.group_reconstruct(grp15, [positions[i] for i in pick], cat([sbs[i]["share"] for i in pick]))
        assert len(gs) == EB and int.from_bytes(mask, "big") ^ box["U"] == want
        assert int.from_bytes(mask, "big") == g.secret_mask(int.from_bytes(gs, "big"))


def test_same_call_through_two_handle_sizes(engine, grp15):
    """one group_batch_exp through a 256-byte handle and one through a wide handle, before and after each other"""
    q14, q15 = H.rfc_prime(2048), WH.group15()
    narrow = ModpGroup(q14)
    rng = random.Random(8)
    Bn, En = [rng.getrandbits(2048) for _ in range(17)], [rng.getrandbits(2048) for _ in range(17)]
    Bw, Ew = [rng.getrandbits(3072) for _ in range(17)], [rng.getrandbits(3072) for _ in range(17)]
    want_n = cat([pow(b, e, q14) for b, e in zip(Bn, En)], 256)
    want_w = cat([pow(b, e, q15) for b, e in zip(Bw, Ew)])
    for _ in range(2):
        assert engine.group_batch_exp(narrow, cat(Bn, 256), cat(En, 256)) == want_n
        assert engine.group_batch_exp(grp15, cat(Bw), cat(Ew)) == want_w
    assert (narrow.elem_bytes, grp15.elem_bytes) == (256, 384)
    narrow.close()
