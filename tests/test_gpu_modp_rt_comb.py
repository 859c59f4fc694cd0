"""Fixed-base comb of a run-time MODP group on the GPU (k_rt_comb_bases / k_rt_comb_rows / k_rt_comb_exp behind
mpvss_modp_group_batch_exp_fixed_base, _prepare and the protocol entry points): byte parity with Python's pow and with the
per-share-base path group_batch_exp (the base repeated), the dual form through group_dleq_commitments, the protocol on a fresh
and on a prepared context against the oracle, the crossover, the context's comb cache and the error contract.

A base other than the generators gets its comb the way an application does: one call of comb_min_shares exponents (all of
them 1, so the call costs the build and little else); the small calls that follow hit the cached table, which the counters of
group_comb_stats confirm."""
import ctypes as C
import random
import threading

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
from mpvss_rs_amd import Engine, ModpGroup, capi

pytestmark = pytest.mark.gpu

EB = 256
TOP = (1 << 2048) - 1
E_INVALID = -1


def enc(v):
    return (v % (1 << 2048)).to_bytes(EB, "big")


def cat(vals):
    return b"".join(enc(v) for v in vals)


def split(b):
    return [int.from_bytes(b[i:i + EB], "big") for i in range(0, len(b), EB)]


def _prime(bits):
    return H.rfc_prime(bits) if bits in H.RFC_C else H.small_safe_primes()[bits]


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own: the comb counters start at zero and no other test's tables are in its cache"""
    e = Engine(0)
    yield e
    e.close()


def _min_shares(grp):
    m = grp.comb_min_shares
    assert 1 <= m <= 65536, m
    return m


def _build_comb(e, grp, base):
    """the comb of (q, base) through the public interface: one call at the crossover size, every exponent 1"""
    m = _min_shares(grp)
    before = e.group_comb_stats()
    out = e.group_batch_exp_fixed_base(grp, enc(base), enc(1) * m)
    assert out == enc(base % grp.q) * m
    after = e.group_comb_stats()
    assert after["builds"] + after["hits"] == before["builds"] + before["hits"] + 1
    return after


_POW = {}


def _pow(base, x, q):
    """Python's pow, computed once per operand triple (the sliced calls of one base share their exponents)"""
    key = (base, x, q)
    if key not in _POW:
        _POW[key] = pow(base, x, q)
    return _POW[key]


def _fixed(e, grp, base, exps):
    """group_batch_exp_fixed_base over the cached comb (a hit is asserted), checked against both references"""
    before = e.group_comb_stats()
    got = e.group_batch_exp_fixed_base(grp, enc(base), cat(exps))
    after = e.group_comb_stats()
    assert after["hits"] == before["hits"] + 1 and after["builds"] == before["builds"], "the call did not run over the comb"
    assert split(got) == [_pow(base, x, grp.q) for x in exps]
    assert got == e.group_batch_exp(grp, enc(base) * len(exps), cat(exps))
    return got


def _special_waves(rng):
    mixed = [5, rng.getrandbits(2048) | (1 << 2047)] + [rng.getrandbits(rng.choice((3, 64, 2048))) for _ in range(14)]
    skip = [sum(rng.randrange(16) << (4 * w) for w in range(0, 512, 3)) for _ in range(16)]
    top_only = [0] * 16
    top_only[11] = 9 << (4 * 511)
    return [mixed, skip, top_only]


@pytest.mark.parametrize("bits", [40, 256, 1024, 1536, 2048])
def test_fixed_base_parity(eng, bits):
    q = _prime(bits)
    grp = ModpGroup(q)
    assert grp.limbs_per_lane == {40: 5, 256: 5, 1024: 9, 1536: 18, 2048: 18}[bits]
    rng = random.Random(bits)
    unit = rng.randrange(2, q - 1)
    above = q + 12345 if q + 12345 <= TOP else TOP
    for base in (4, 2, 1, unit, above, q):
        _build_comb(eng, grp, base)
        pool = [0, 1, 15, 16, 1 << 2047, TOP, q - 1, q - 2] + [rng.randrange(q + 1, 1 << 2048) for _ in range(25)]
        for n in (1, 15, 16, 17, 33):
            exps = [pool[(n + i) % len(pool)] for i in range(n)]
            _fixed(eng, grp, base, exps)
        for wave in _special_waves(rng):
            _fixed(eng, grp, base, wave + wave[:1])            # the wave, and a second workgroup with 15 dead quads
    _POW.clear()


@pytest.mark.parametrize("bits", [256, 1024, 2048])
def test_dual_form_through_dleq_commitments(bits):
    q = _prime(bits)
    grp = ModpGroup(q)
    rng = random.Random(bits + 1)
    e = Engine(0)
    try:
        e.group_prepare(grp)
        assert e.group_comb_stats() == {"builds": 2, "hits": 0, "evictions": 0}
        hits = 0
        for g1, sizes in ((4, (1, 16, 17)), (2, (16,))):
            for n in sizes:
                h1 = [rng.randrange(1 << 2048) for _ in range(n)]
                h1[n // 2] = q                                              # 0 mod q
                g2, h2 = ([rng.randrange(1 << 2048) for _ in range(n)] for _ in range(2))
                r = [rng.randrange(1 << 2048) for _ in range(n)]
                r[-1] = 0
                shared = [0, 1, rng.getrandbits(256) | (1 << 255), TOP]
                cases = [[v] * n for v in shared] + [[rng.randrange(1 << rng.choice((1, 256, 2048))) for _ in range(n)]]
                for k, c in enumerate(cases):
                    per_share = len(set(c)) > 1 or n == 1 and c[0] not in shared
                    a1, a2 = e.group_dleq_commitments(grp, enc(g1), cat(h1), cat(g2), cat(h2), cat(r), cat(c) if per_share else enc(c[0]),
                                                      per_share)
                    hits += 1
                    assert e.group_comb_stats() == {"builds": 2, "hits": hits, "evictions": 0}
                    assert split(a1) == [pow(g1, x, q) * pow(h, y, q) % q for x, h, y in zip(r, h1, c)], (g1, n, c[0])
                    if k in (2, 4):          # a2 does not run over a comb: two of its cases are enough beside the rest of the suite
                        assert split(a2) == [pow(g, x, q) * pow(h, y, q) % q for g, x, h, y in zip(g2, r, h2, c)]
    finally:
        e.close()


def _instance(q, n, t, seed):
    g = H.RtOracleGroup(q)
    rng = random.Random(seed)
    privs, pks, seen = [], [], set()
    while len(pks) < n:
        k = H.keygen(g, rng)
        pk = g.generate_public_key(k)
        if pk not in seen:
            seen.add(pk)
            privs.append(k)
            pks.append(pk)
    coeffs = [rng.randrange(g.q - 1) for _ in range(t)]
    coeffs[0] = coeffs[0] or 1
    ws = [H.keygen(g, rng) for _ in range(n)]
    w2 = [H.keygen(g, rng) for _ in range(n)]
    box = O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)
    return g, privs, pks, coeffs, ws, w2, box


def _protocol(e, g, grp, privs, pks, coeffs, ws, w2, box):
    n = len(pks)
    positions = list(range(1, n + 1))
    keys = [g.element_to_bytes(p) for p in pks]
    deal = e.group_deal(grp, cat(coeffs), positions, cat(pks), cat(ws))
    flat = O.box_to_flat(g, box)
    ver = e.group_verify_distribution(grp, flat["commitments"], positions, cat(pks), deal["Y"], deal["responses"], deal["challenge"],
                                      dump=True)
    bad = bytearray(deal["responses"])
    bad[EB + 200] ^= 1
    ver_bad = e.group_verify_distribution(grp, flat["commitments"], positions, cat(pks), deal["Y"], bytes(bad), deal["challenge"])
    Y = cat([box["shares"][k] for k in keys])
    xinv = [O.mod_inverse(k, g.q - 1) for k in privs]
    S, Cc = e.group_extract_shares(grp, cat(pks), Y, cat(xinv), cat(w2))
    R = capi.group_dleq_responses(grp, cat(w2), cat(privs), Cc)
    vs = bytes(e.group_verify_shares(grp, cat(pks), S, Y, Cc, R))
    Rbad = bytearray(R)
    Rbad[3 * EB + 255] ^= 1
    vs_bad = bytes(e.group_verify_shares(grp, cat(pks), S, Y, Cc, bytes(Rbad)))
    return {"deal": deal, "ver": ver, "ver_bad": ver_bad, "S": S, "C": Cc, "R": R, "vs": vs, "vs_bad": vs_bad}


@pytest.mark.parametrize("bits", [256, 1024, 2048])
def test_protocol_fresh_and_prepared_against_the_oracle(bits):
    q = _prime(bits)
    grp = ModpGroup(q)
    n, t = 17, 5
    g, privs, pks, coeffs, ws, w2, box = _instance(q, n, t, seed=bits)
    keys = [g.element_to_bytes(p) for p in pks]
    e = Engine(0)
    try:
        fresh = _protocol(e, g, grp, privs, pks, coeffs, ws, w2, box)
        s0 = e.group_comb_stats()
        if _min_shares(grp) > n:
            assert s0 == {"builds": 0, "hits": 0, "evictions": 0}
        e.group_prepare(grp)
        s1 = e.group_comb_stats()
        prepared = _protocol(e, g, grp, privs, pks, coeffs, ws, w2, box)
        s2 = e.group_comb_stats()
    finally:
        e.close()
    assert fresh == prepared
    assert s2["builds"] == s1["builds"] and s2["evictions"] == 0
    # deal: X and a1 over g; two verify_distribution: a1; extract: a1 over G; two verify_shares: a1
    assert s2["hits"] - s1["hits"] == 7
    d = prepared["deal"]
    assert split(d["X"]) == box["_X"] and split(d["a1"]) == box["_a1"] and split(d["a2"]) == box["_a2"]
    assert split(d["Y"]) == [box["shares"][k] for k in keys] and d["digest"] == box["_digest"]
    assert split(d["challenge"]) == [box["challenge"]] and split(d["responses"]) == [box["responses"][k] for k in keys]
    v = prepared["ver"]
    assert v["verdict"] is True and v["digest"] == box["_digest"] and v["X"] == d["X"] and v["a1"] == d["a1"] and v["a2"] == d["a2"]
    assert prepared["ver_bad"]["verdict"] is False
    sbs = [O.extract_secret_share(g, box, k, w) for k, w in zip(privs, w2)]
    assert split(prepared["S"]) == [sb["share"] for sb in sbs] and split(prepared["C"]) == [sb["challenge"] for sb in sbs]
    assert split(prepared["R"]) == [sb["response"] for sb in sbs]
    assert prepared["vs"] == bytes([1] * n) and prepared["vs_bad"] == bytes([1, 1, 1, 0] + [1] * (n - 4))


def test_crossover():
    q = _prime(256)
    grp = ModpGroup(q)
    m = _min_shares(grp)
    rng = random.Random(5)

    def exps(n):
        return [rng.getrandbits(2048) if i < 40 else rng.getrandbits(16) for i in range(n)]

    e = Engine(0)
    try:
        if m > 1:
            x = exps(m - 1)
            assert split(e.group_batch_exp_fixed_base(grp, enc(4), cat(x))) == [pow(4, v, q) for v in x]
            assert e.group_comb_stats() == {"builds": 0, "hits": 0, "evictions": 0}
        x = exps(m)
        assert split(e.group_batch_exp_fixed_base(grp, enc(4), cat(x))) == [pow(4, v, q) for v in x]
        assert e.group_comb_stats() == {"builds": 1, "hits": 0, "evictions": 0}
        x = [rng.getrandbits(2048)]
        assert split(e.group_batch_exp_fixed_base(grp, enc(4), cat(x))) == [pow(4, x[0], q)]
        assert e.group_comb_stats() == {"builds": 1, "hits": 1, "evictions": 0}
    finally:
        e.close()


def test_cache_eviction_handles_and_contexts():
    q = _prime(256)
    grp = ModpGroup(q)
    rng = random.Random(6)
    x = [rng.getrandbits(2048) for _ in range(17)]
    e = Engine(0)
    e2 = Engine(0)
    try:
        pairs = [(grp, 3), (grp, 5), (ModpGroup(_prime(64)), 3), (grp, 7), (ModpGroup(_prime(1024)), 3)]
        for k, (gp, base) in enumerate(pairs):
            s = _build_comb(e, gp, base)
            assert s["builds"] == k + 1 and s["evictions"] == (1 if k == 4 else 0)
        # the least recently used pair (q, 3) went; the others still hit; (q, 3) is rebuilt and right
        for gp, base in pairs[1:]:
            _fixed(e, gp, base, x)
        before = e.group_comb_stats()
        got = e.group_batch_exp_fixed_base(grp, enc(3), cat(x))
        assert split(got) == [pow(3, v, q) for v in x]
        if _min_shares(grp) > len(x):
            assert e.group_comb_stats() == before                       # a small call of an evicted pair builds nothing
        s = _build_comb(e, grp, 3)
        assert s["builds"] == 6 and s["evictions"] == 2
        _fixed(e, grp, 3, x)
        # a destroyed handle and a new one for another modulus (its address may be the old one): the key is (q, base)
        q1, q2 = _prime(512), _prime(768)
        g1 = ModpGroup(q1)
        e.group_prepare(g1)
        assert split(e.group_batch_exp_fixed_base(g1, enc(4), cat(x))) == [pow(4, v, q1) for v in x]
        g1.close()
        g2 = ModpGroup(q2)
        assert split(e.group_batch_exp_fixed_base(g2, enc(4), cat(x))) == [pow(4, v, q2) for v in x]
        e.group_prepare(g2)
        assert split(e.group_batch_exp_fixed_base(g2, enc(4), cat(x))) == [pow(4, v, q2) for v in x]
        # two contexts, one handle
        e2.group_prepare(g2)
        assert e2.group_comb_stats() == {"builds": 2, "hits": 0, "evictions": 0}
        assert e2.group_batch_exp_fixed_base(g2, enc(2), cat(x)) == e.group_batch_exp_fixed_base(g2, enc(2), cat(x)) == \
            cat([pow(2, v, q2) for v in x])
    finally:
        e.close()
        e2.close()


def test_four_threads_alternate_two_groups():
    groups = [ModpGroup(_prime(256)), ModpGroup(_prime(1024))]
    rng = random.Random(7)
    jobs = []
    for k in range(8):
        grp = groups[k % 2]
        n = 5 + k
        x, h, r = ([rng.getrandbits(2048) for _ in range(n)] for _ in range(3))
        c = rng.getrandbits(256)
        want = (cat([pow(2, v, grp.q) for v in x]),
                cat([pow(4, a, grp.q) * pow(b, c, grp.q) % grp.q for a, b in zip(r, h)]))
        jobs.append((grp, x, h, r, c, want))
    e = Engine(0)
    got, errors = [None] * len(jobs), []

    def work(idx):
        try:
            for k in idx:
                grp, x, h, r, c, _ = jobs[k]
                if k < 4:
                    e.group_prepare(grp)
                pk = e.group_batch_exp_fixed_base(grp, enc(2), cat(x))
                a1, _a2 = e.group_dleq_commitments(grp, enc(4), cat(h), cat(h), cat(h), cat(r), enc(c), False)
                got[k] = (pk, a1)
        except Exception as ex:      # noqa: BLE001
            errors.append(ex)

    try:
        th = [threading.Thread(target=work, args=(list(range(i, len(jobs), 4)),)) for i in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        stats = e.group_comb_stats()
    finally:
        e.close()
    assert not errors, errors
    assert got == [j[5] for j in jobs]
    assert stats["builds"] == 4 and stats["evictions"] == 0 and stats["hits"] >= 16


def test_errors_and_the_empty_call(eng):
    grp = ModpGroup(_prime(256))
    lib = eng.lib
    fb = lib.mpvss_modp_group_batch_exp_fixed_base
    base = (C.c_uint8 * EB).from_buffer_copy(enc(4))
    exps = (C.c_uint8 * EB).from_buffer_copy(enc(5))
    out = (C.c_uint8 * EB)(*([0xA5] * EB))
    pb, pe, po = (C.cast(a, C.c_void_p) for a in (base, exps, out))
    before = eng.group_comb_stats()
    assert fb(eng.ctx, grp.handle, capi.MPVSS_HOST, None, pe, 1, po) == E_INVALID
    assert fb(eng.ctx, grp.handle, capi.MPVSS_HOST, pb, None, 1, po) == E_INVALID
    assert fb(eng.ctx, grp.handle, capi.MPVSS_HOST, pb, pe, 1, None) == E_INVALID
    assert fb(eng.ctx, None, capi.MPVSS_HOST, pb, pe, 1, po) == E_INVALID
    assert fb(None, grp.handle, capi.MPVSS_HOST, pb, pe, 1, po) == E_INVALID
    assert lib.mpvss_modp_group_prepare(eng.ctx, None) == E_INVALID and lib.mpvss_modp_group_prepare(None, grp.handle) == E_INVALID
    assert lib.mpvss_modp_group_comb_min_shares(None) == E_INVALID
    assert lib.mpvss_modp_group_comb_stats(None, None, None, None) == E_INVALID
    assert lib.mpvss_modp_group_comb_stats(eng.ctx, None, None, None) == 0
    # n == 0: fine, and nothing is touched (null pointers are allowed then)
    assert fb(eng.ctx, grp.handle, capi.MPVSS_HOST, pb, pe, 0, po) == 0
    assert fb(eng.ctx, grp.handle, capi.MPVSS_HOST, None, None, 0, None) == 0
    assert bytes(out) == bytes([0xA5] * EB) and eng.group_comb_stats() == before
    assert eng.group_batch_exp_fixed_base(grp, enc(4), b"") == b""
    # the context still works after the refusals
    assert split(eng.group_batch_exp_fixed_base(grp, enc(4), enc(5))) == [1024]
