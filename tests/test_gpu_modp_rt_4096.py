"""Run-time MODP groups of 512-byte elements on the GPU (mpvss_modp_group_create_wide with elem_bytes 512: 36 limbs per lane,
moduli of 3073 .. 4096 bits): exp / mul / twin / fixed base against Python's pow at the share counts around one workgroup's 16
numbers, both sides of the comb and twin launch decisions, the whole protocol on RFC 3526 group 16 against the oracle over
RtOracleGroup, one small case of every other feature of a run-time group at this width, and the three handle sizes side by
side in one process.

References.  A 4096-bit pow of Python's integers takes 0.15 - 0.25 s, so the powers of the edge operands are computed once per
modulus (pool(): every base with every exponent) and every test draws its rows from that pool, at changing batch sizes and
lanes; the rows that fill a batch beyond it have short exponents, whose pow is cheap.  The oracle's protocol runs (some 600
such pows) are XH.protocol_run's, computed once per process and shared by the tests that need them."""
import functools
import hashlib
import random

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import modp_rt_4096_helpers as XH
from mpvss_rs_amd import Engine, ModpGroup, capi

pytestmark = pytest.mark.gpu

EB, TOP = XH.EB, XH.TOP
cat, split, be = XH.cat, XH.split, XH.be
SIZES = (1, 15, 16, 17, 33)          # one workgroup's 16 numbers, one less, one more, and a ragged tail
MODULI = {"group16": XH.group16, "2^4096-1": lambda: TOP, "odd3073": XH.odd_3073}


@pytest.fixture(scope="module", params=sorted(MODULI))
def wide(request):
    q = MODULI[request.param]()
    grp = ModpGroup(q, elem_bytes=EB)
    assert (grp.elem_bytes, grp.limbs_per_lane) == (512, 36)
    yield request.param, q, grp
    grp.close()


@pytest.fixture(scope="module")
def grp16():
    grp = ModpGroup(XH.group16(), elem_bytes=EB)
    yield grp
    grp.close()


def _bases(q, rng):
    """0, 1, q - 1, q, q + 1, 2^4096 - 1 (q + 1 has no 512-byte encoding when q = 2^4096 - 1) and a random one"""
    return [b for b in (0, 1, q - 1, q, q + 1) if b <= TOP] + [TOP, rng.getrandbits(4096)]


def _exps(q, rng):
    """0, 1, q - 1, 2^4096 - 1, only the top nibble, only bit 3072 (the first bit a 384-byte edge would lose), random"""
    return [0, 1, q - 1, TOP, 0xF << 4092, 1 << 3072, rng.getrandbits(4096)]


@functools.lru_cache(maxsize=None)
def pool(name):
    """(bases, exponents, {(base, exponent): pow}) of a modulus: every edge base with every edge exponent, computed once"""
    q = MODULI[name]()
    rng = random.Random(q & 0xFFFF)
    bases, exps = _bases(q, rng), _exps(q, rng)
    return bases, exps, {(b, e): pow(b, e, q) for b in bases for e in exps}


def _short(rng):
    """an exponent whose pow is cheap for any base"""
    return rng.getrandbits(rng.choice((1, 8, 64)))


def _batches(rows, rng, fill):
    """rows cut into batches of SIZES, in turn, the last one filled up with fill(rng)"""
    out, i, k = [], 0, 0
    while i < len(rows) or k < len(SIZES):
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
    name, q, grp = wide
    bases, exps, ref = pool(name)
    rng = random.Random(1)
    rows = [(b, e) for b in bases for e in exps]
    rng.shuffle(rows)
    seen = 0
    for chunk in _batches(rows, rng, lambda r: (r.getrandbits(4096), _short(r))):
        B, E = zip(*chunk)
        out = engine.group_batch_exp(grp, cat(B), cat(E))
        assert len(out) == len(B) * EB
        assert split(out) == [ref[(b, e)] if (b, e) in ref else pow(b, e, q) for b, e in zip(B, E)], len(B)
        seen += len(B)
    assert seen >= len(rows) and seen >= sum(SIZES)


def test_mixed_lengths_within_one_wave(engine, wide):
    """the wave's highest bit comes from one lane only: every other number of the wave idles through its windows"""
    name, q, grp = wide
    bases, exps, ref = pool(name)
    rng = random.Random(2)
    rnd = bases[-1]
    for long_row, long_e in ((5, TOP), (0, 0xF << 4092), (15, 1 << 3072)):
        E = [_short(rng) for _ in range(16)]
        E[long_row] = long_e
        E[(long_row + 3) % 16] = 0
        B = [rng.getrandbits(4096) for _ in range(16)]
        B[long_row] = rnd
        want = [ref[(b, e)] if (b, e) in ref else pow(b, e, q) for b, e in zip(B, E)]
        assert split(engine.group_batch_exp(grp, cat(B), cat(E))) == want
        E2 = [_short(rng) for _ in range(16)]                 # the second exponent set: short but for the same lane
        E2[long_row] = q - 1
        o1, o2 = engine.group_batch_twin_exp(grp, cat(B), cat(E), cat(E2))
        assert split(o1) == want
        assert split(o2) == [ref[(b, e)] if (b, e) in ref else pow(b, e, q) for b, e in zip(B, E2)]
        assert split(engine.group_batch_exp_fixed_base(grp, be(rnd), cat(E))) == [ref[(rnd, e)] if (rnd, e) in ref else pow(rnd, e, q)
                                                                                  for e in E]


def test_batch_mul_matches_python(engine, wide):
    name, q, grp = wide
    rng = random.Random(3)
    vals = pool(name)[0][:-1] + [q - 2, 2, 1 << 3072]
    rows = [(a, b) for a in vals for b in vals]
    for chunk in _batches(rows, rng, lambda r: (r.getrandbits(4096), r.getrandbits(4096))):
        A, B = zip(*chunk)
        assert split(engine.group_batch_mul(grp, cat(A), cat(B))) == [a * b % q for a, b in zip(A, B)], len(A)


def test_batch_twin_exp_matches_pow(engine, wide):
    name, q, grp = wide
    bases, exps, ref = pool(name)
    rng = random.Random(4)
    rows = [(b, exps[i % len(exps)], exps[(i // 2 + 3 * k) % len(exps)]) for k, b in enumerate(bases) for i in range(len(exps))]
    rng.shuffle(rows)
    for chunk in _batches(rows, rng, lambda r: (r.getrandbits(4096), _short(r), _short(r))):
        B, E1, E2 = zip(*chunk)
        o1, o2 = engine.group_batch_twin_exp(grp, cat(B), cat(E1), cat(E2))
        assert split(o1) == [ref[(b, e)] if (b, e) in ref else pow(b, e, q) for b, e in zip(B, E1)], len(B)
        assert split(o2) == [ref[(b, e)] if (b, e) in ref else pow(b, e, q) for b, e in zip(B, E2)], len(B)


def test_batch_exp_fixed_base_matches_pow(engine, wide):
    """below comb_min_shares on a context that has no comb of these bases: the 16-entry table path"""
    name, q, grp = wide
    bases, exps, ref = pool(name)
    rng = random.Random(5)
    assert max(SIZES) < grp.comb_min_shares
    for k, base in enumerate(bases):
        n = SIZES[k % len(SIZES)]
        E = (exps[k % len(exps):] + exps + [_short(rng) for _ in range(n)])[:n]
        out = engine.group_batch_exp_fixed_base(grp, be(base), cat(E))
        assert split(out) == [ref[(base, e)] if (base, e) in ref else pow(base, e, q) for e in E], (k, n)


def test_fixed_base_on_both_sides_of_the_launch_decision():
    """two 512-byte groups and one 256-byte group on ONE context of their own: without prepare a small call takes the 16-entry
    table (no build, no hit); after prepare the comb (hit), same bytes; the cache keeps (q, base) of the three groups apart"""
    eng = Engine(0)
    rng = random.Random(6)
    qa, qb, qc = XH.group16(), XH.odd_3073(), H.rfc_prime(2048)
    ga, gb, gc = ModpGroup(qa, elem_bytes=EB), ModpGroup(qb, elem_bytes=EB), ModpGroup(qc)
    try:
        n = 33
        assert n < ga.comb_min_shares and n < gc.comb_min_shares
        Ew = [0, 1, TOP, 0xF << 4092, 1 << 3072] + [_short(rng) for _ in range(n - 5)]
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
        E2 = Ew[:8]
        assert eng.group_batch_exp_fixed_base(ga, be(2), cat(E2)) == cat([pow(2, e, qa) for e in E2])
    finally:
        for g in (ga, gb, gc):
            g.close()
        eng.close()


def test_twin_on_both_sides_of_its_crossover(engine, grp16):
    """k_rt_twin_exp at twin_min_shares shares, once; the same rows through the two exponent sets in calls below the
    crossover: equal bytes everywhere, and equal to pow on 64 positions -- the pool's rows, which stand at every seventh
    position, and rows with short exponents between them"""
    q = XH.group16()
    bases, exps, ref = pool("group16")
    m = grp16.twin_min_shares
    assert 33 < m <= 24576 and m % 2 == 0, f"twin_min_shares = {m}: this test needs the default build's constant"
    rng = random.Random(7)
    rows = [(b, e1, e2) for b in bases for e1 in exps for e2 in exps[::3]]
    B, E1, E2 = [], [], []
    for i in range(m):
        if i % 7 == 0 or i < 36:
            b, e1, e2 = rows[(i * 5 + i // 7) % len(rows)]
        else:
            b, e1, e2 = rng.getrandbits(4096), _short(rng), _short(rng)
        B.append(b), E1.append(e1), E2.append(e2)
    cb, c1, c2 = cat(B), cat(E1), cat(E2)
    big = engine.group_batch_twin_exp(grp16, cb, c1, c2)
    small = engine.group_batch_twin_exp(grp16, cb[:33 * EB], c1[:33 * EB], c2[:33 * EB])
    assert big[0][:33 * EB] == small[0] and big[1][:33 * EB] == small[1]
    half = m // 2 * EB
    lo = engine.group_batch_twin_exp(grp16, cb[:half], c1[:half], c2[:half])
    hi = engine.group_batch_twin_exp(grp16, cb[half:], c1[half:], c2[half:])
    assert big[0] == lo[0] + hi[0] and big[1] == lo[1] + hi[1]
    g1, g2 = split(big[0]), split(big[1])
    idx = sorted(set(list(range(36)) + [m - 1, m - 2] + [rng.randrange(m) for _ in range(40)]))[:64]
    want = lambda b, e: ref[(b, e)] if (b, e) in ref else pow(b, e, q)
    assert [g1[i] for i in idx] == [want(B[i], E1[i]) for i in idx]
    assert [g2[i] for i in idx] == [want(B[i], E2[i]) for i in idx]


# ---- the protocol on group 16 ----------------------------------------------------------------------------------------
golden = XH.protocol_run
SHAPES = ((5, 3), (33, 4))


def _flip(buf, row, byte=EB - 1):
    b = bytearray(buf)
    b[row * EB + byte] ^= 1
    return bytes(b)


@pytest.mark.parametrize("n,t", SHAPES)
def test_protocol_on_group16_against_the_oracle(engine, grp16, n, t):
    q = XH.group16()
    G = golden(n, t)
    g = H.RtOracleGroup(q)
    positions = list(range(1, n + 1))
    pks, coeffs, ws = G["pks"], G["coeffs"], G["ws"]
    # deal: every byte of the box and of the proofs
    res = engine.group_deal(grp16, cat(coeffs), positions, cat(pks), cat(ws))
    assert split(res["X"]) == G["X"] and split(res["a1"]) == G["a1"] and split(res["a2"]) == G["a2"]
    assert split(res["Y"]) == G["Y"]
    assert res["digest"] == G["digest"]
    assert split(res["challenge"]) == [G["challenge"]]
    assert split(res["responses"]) == G["responses"]
    C = cat(G["commitments"])
    assert split(engine.group_batch_exp_fixed_base(grp16, be(4), cat(coeffs))) == G["commitments"]
    # verify_distribution, and one flipped byte of one Y_i / of one response
    v = engine.group_verify_distribution(grp16, C, positions, cat(pks), res["Y"], res["responses"], res["challenge"], dump=True)
    assert v["verdict"] is True and v["digest"] == res["digest"]
    assert (v["X"], v["a1"], v["a2"]) == (res["X"], res["a1"], res["a2"])
    assert G["tampered_valid"] in (False, None)                  # (the oracle is asked about the flipped share at (5, 3) only)
    for bad_y, bad_r in ((_flip(res["Y"], XH.TAMPER_ROW), res["responses"]), (_flip(res["Y"], n // 2, 0), res["responses"]),
                         (res["Y"], _flip(res["responses"], n - 1, 17))):
        assert engine.group_verify_distribution(grp16, C, positions, cat(pks), bad_y, bad_r, res["challenge"])["verdict"] is False
    # distribute with the commitments (Horner in the exponent over t of them)
    P = [O.poly_get_value(coeffs, i) % (q - 1) for i in positions]
    d = engine.group_distribute(grp16, C, positions, cat(pks), cat(P), cat(ws))
    assert all(d[k] == res[k] for k in ("X", "Y", "a1", "a2", "digest"))
    # extract_secret_share and its proofs
    xinv = [O.mod_inverse(k, q - 1) for k in G["privs"]]
    S, Cs = engine.group_extract_shares(grp16, cat(pks), res["Y"], cat(xinv), cat(G["w2"]))
    assert split(S) == G["share"] and split(Cs) == G["share_challenge"]
    R = capi.group_dleq_responses(grp16, cat(G["w2"]), cat(G["privs"]), Cs)
    assert split(R) == G["share_response"]
    assert list(engine.group_verify_shares(grp16, cat(pks), S, res["Y"], Cs, R)) == [1] * n
    bad = n // 3
    assert list(engine.group_verify_shares(grp16, cat(pks), _flip(S, bad), res["Y"], Cs, R)) == [int(i != bad) for i in range(n)]
    assert list(engine.group_verify_shares(grp16, cat(pks), S, res["Y"], Cs, _flip(R, n - 1, 200))) == [1] * (n - 1) + [0]
    # reconstruct from all n shares, from exactly t spread ones, from the first and from the last t
    assert len(G["reconstructed"]) == 4
    for pick, want in G["reconstructed"]:
        assert want == XH.SECRET
        gs, mask = engine.group_reconstruct(grp16, [positions[i] for i in pick], cat([G["share"][i] for i in pick]))
        assert len(gs) == EB and int.from_bytes(mask, "big") ^ G["U"] == want
        assert int.from_bytes(mask, "big") == g.secret_mask(int.from_bytes(gs, "big"))


# ---- one small case of every other feature at 512 bytes, against the same runs of the oracle --------------------------------
@pytest.fixture()
def own_engine():
    eng = Engine(0)
    yield eng
    eng.close()


def test_forward_differences_switched_on(own_engine, grp16):
    G = golden(33, 4)
    positions = list(range(1, 34))
    C = cat(G["commitments"])
    own_engine.set_rt_fd(2, 0)
    before = own_engine.group_fd_stats()
    assert split(own_engine.group_commit_eval(grp16, C, positions)) == G["X"]
    after = own_engine.group_fd_stats()
    assert (after["fd"] - before["fd"], after["horner"] - before["horner"]) == (1, 0)
    own_engine.set_rt_fd(2, 2)                                           # two chains of 16 and 17 positions
    assert split(own_engine.group_commit_eval(grp16, C, positions)) == G["X"]
    v = own_engine.group_verify_distribution(grp16, C, positions, cat(G["pks"]), cat(G["Y"]), cat(G["responses"]), be(G["challenge"]))
    assert v["verdict"] is True and v["digest"] == G["digest"]
    assert own_engine.group_fd_stats()["fd"] - before["fd"] == 3
    own_engine.set_rt_fd(0, 0)
    assert split(own_engine.group_commit_eval(grp16, C, positions)) == G["X"]
    assert own_engine.group_fd_stats()["horner"] - before["horner"] == 1


def test_device_scalar_ring_switched_on(own_engine, grp16):
    q = XH.group16()
    G = golden(5, 3)
    positions = list(range(1, 6))
    assert grp16.has_device_scalar
    own_engine.set_rt_scalar(2)
    before = own_engine.group_scalar_stats()
    res = own_engine.group_deal(grp16, cat(G["coeffs"]), positions, cat(G["pks"]), cat(G["ws"]))
    assert split(res["responses"]) == G["responses"] and split(res["Y"]) == G["Y"] and res["digest"] == G["digest"]
    xinv = [O.mod_inverse(k, q - 1) for k in G["privs"]]
    S, Cs = own_engine.group_extract_shares(grp16, cat(G["pks"]), cat(G["Y"]), cat(xinv), cat(G["w2"]))
    assert split(S) == G["share"] and split(Cs) == G["share_challenge"]
    after = own_engine.group_scalar_stats()
    assert (after["device"] - before["device"], after["host"] - before["host"]) == (2, 0)
    # the ring's own entry point at the edges of the operands
    ops = [q - 2, 0, 1, q - 1, q, TOP, G["w2"][0]]
    A, B = [a for a in ops for _ in ops], [b for _ in ops for b in ops]
    assert split(own_engine.group_batch_scalar_mul(grp16, cat(A), cat(B))) == [a * b % (q - 1) for a, b in zip(A, B)]


def test_device_share_hash_against_the_host_hash(own_engine, grp16):
    G = golden(33, 4)
    g = H.RtOracleGroup(XH.group16())
    n = 33
    assert grp16.has_device_share_hash
    # any four elements per share, zero and a one-byte value among them (the framing is of minimal length)
    h1, h2, a1, a2 = list(G["pks"]), list(G["Y"]), list(G["a1"]), list(G["a2"])
    h1[0], h2[1], a1[2], a2[3], h1[4] = 0, 1, 255, 256, TOP
    got = split(own_engine.group_dleq_challenges(grp16, cat(h1), cat(h2), cat(a1), cat(a2)))
    want = [g.hash_to_scalar(hashlib.sha256(O.append_transcript(g, *row)).digest()) for row in zip(h1, h2, a1, a2)]
    assert got == want
    assert got == [int.from_bytes(grp16.hash_to_scalar(hashlib.sha256(O.append_transcript(g, *row)).digest()), "big")
                   for row in zip(h1, h2, a1, a2)]
    # verify_shares with the hash on the device and on the host: the oracle's proofs pass, a flipped byte fails, either way
    S, Y, Cs, R, pk = cat(G["share"]), cat(G["Y"]), cat(G["share_challenge"]), cat(G["share_response"]), cat(G["pks"])
    for mode, where in ((2, "device"), (0, "host")):
        own_engine.set_rt_share_hash(mode)
        before = own_engine.group_share_hash_stats()
        assert list(own_engine.group_verify_shares(grp16, pk, S, Y, Cs, R)) == [1] * n
        assert list(own_engine.group_verify_shares(grp16, pk, _flip(S, 17), Y, Cs, R)) == [int(i != 17) for i in range(n)]
        after = own_engine.group_share_hash_stats()
        assert after[where] - before[where] == 2 and sum(after.values()) - sum(before.values()) == 2


def test_a_key_set_of_17_keys(own_engine, grp16):
    q = XH.group16()
    G = golden(33, 4)
    k0, nk = 5, 17                                                          # the keys of the shares 6 .. 22
    ks = own_engine.group_keyset_create(grp16, cat(G["pks"][k0:k0 + nk]))
    try:
        P = [O.poly_get_value(G["coeffs"], i) % (q - 1) for i in range(1, 34)]
        Y, a2 = own_engine.group_keyset_twin_exp(grp16, ks, 0, cat(P[k0:k0 + nk]), cat(G["ws"][k0:k0 + nk]))
        assert split(Y) == G["Y"][k0:k0 + nk] and split(a2) == G["a2"][k0:k0 + nk]
        # y^r Y^c, the verifier's a2, over the last 16 keys of the set and over a single one
        for off, m in ((1, 16), (16, 1)):
            sl = slice(k0 + off, k0 + off + m)
            out = own_engine.group_keyset_dual_exp(grp16, ks, off, cat(G["responses"][sl]), cat(G["Y"][sl]), be(G["challenge"]))
            assert split(out) == G["a2"][sl]
        positions = list(range(k0 + 1, k0 + nk + 1))
        sl = slice(k0, k0 + nk)
        # the 17 shares as a box of their own have another transcript: its verdict is the hash's, its a1 / a2 / X the oracle's
        v = own_engine.group_verify_distribution_keyset(grp16, cat(G["commitments"]), positions, ks, 0, cat(G["Y"][sl]),
                                                        cat(G["responses"][sl]), be(G["challenge"]), dump=True)
        assert (split(v["X"]), split(v["a1"]), split(v["a2"])) == (G["X"][sl], G["a1"][sl], G["a2"][sl])
        plain = own_engine.group_verify_distribution(grp16, cat(G["commitments"]), positions, cat(G["pks"][sl]), cat(G["Y"][sl]),
                                                     cat(G["responses"][sl]), be(G["challenge"]))
        assert (v["verdict"], v["digest"]) == (plain["verdict"], plain["digest"]) and v["verdict"] is False
        d = own_engine.group_deal_keyset(grp16, cat(G["coeffs"]), positions, ks, 0, cat(G["ws"][sl]))
        assert (split(d["X"]), split(d["Y"]), split(d["a1"]), split(d["a2"])) == (G["X"][sl], G["Y"][sl], G["a1"][sl], G["a2"][sl])
        assert grp16.keyset_bytes_per_key == 147456
    finally:
        ks.close()


def test_verify_many_with_three_boxes(own_engine, grp16):
    G = golden(5, 3)
    positions = list(range(1, 6))
    box = dict(commitments=cat(G["commitments"]), positions=positions, pubkeys=cat(G["pks"]), shares=cat(G["Y"]),
               responses=cat(G["responses"]), challenge=be(G["challenge"]))
    bad = dict(box, shares=_flip(box["shares"], XH.TAMPER_ROW))
    before = own_engine.group_verify_many_stats()
    got = own_engine.group_verify_many(grp16, [box, bad, box])
    assert [v for v, _ in got] == [True, G["tampered_valid"], True]
    assert got[0][1] == got[2][1] == G["digest"] and got[1][1] != G["digest"]
    one = own_engine.group_verify_distribution(grp16, bad["commitments"], positions, bad["pubkeys"], bad["shares"], bad["responses"],
                                               bad["challenge"])
    assert (one["verdict"], one["digest"]) == got[1]
    after = own_engine.group_verify_many_stats()
    assert after["grouped_boxes"] - before["grouped_boxes"] == 3 and after["single_boxes"] == before["single_boxes"]


def test_reconstruct_many_with_three_secrets(own_engine, grp16):
    G = golden(5, 3)
    g = H.RtOracleGroup(XH.group16())
    picks = [pick for pick, _ in G["reconstructed"] if len(pick) == 3]
    assert len(picks) == 3 and all(want == XH.SECRET for _, want in G["reconstructed"])
    secrets = [dict(positions=[i + 1 for i in pick], shares=cat([G["share"][i] for i in pick])) for pick in picks]
    got = own_engine.group_reconstruct_many(grp16, secrets)
    assert [s for s, _, _ in got] == [0, 0, 0]
    for (_, gs, mask), sec in zip(got, secrets):
        assert int.from_bytes(mask, "big") ^ G["U"] == XH.SECRET
        assert int.from_bytes(mask, "big") == g.secret_mask(int.from_bytes(gs, "big"))
        assert (gs, mask) == own_engine.group_reconstruct(grp16, sec["positions"], sec["shares"])
    assert len({gs for _, gs, _ in got}) == 1                             # G^s whichever three shares


def test_three_handle_sizes_alternately(engine, grp16):
    """one group_batch_exp through a 256-byte, a 384-byte and a 512-byte handle in turn, twice: each gives its own answers"""
    q14, q15, q16 = H.rfc_prime(2048), WH.group15(), XH.group16()
    g14, g15 = ModpGroup(q14), ModpGroup(q15, elem_bytes=384)
    bases, exps, ref = pool("group16")
    rng = random.Random(8)
    rows16 = [(bases[-1], e) for e in exps] + [(TOP, exps[3])] + [(rng.getrandbits(4096), _short(rng)) for _ in range(9)]
    sets = []
    for grp, q, eb, bits in ((g14, q14, 256, 2048), (g15, q15, 384, 3072)):
        rows = [(rng.getrandbits(bits), rng.getrandbits(bits))] + [(rng.getrandbits(bits), _short(rng)) for _ in range(16)]
        sets.append((grp, eb, rows, cat([pow(b, e, q) for b, e in rows], eb)))
    sets.append((grp16, 512, rows16, cat([ref[(b, e)] if (b, e) in ref else pow(b, e, q16) for b, e in rows16])))
    for _ in range(2):
        for grp, eb, rows, want in sets:
            B, E = zip(*rows)
            assert engine.group_batch_exp(grp, cat(B, eb), cat(E, eb)) == want
    assert (g14.elem_bytes, g15.elem_bytes, grp16.elem_bytes) == (256, 384, 512)
    g14.close()
    g15.close()
