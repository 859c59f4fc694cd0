"""Key sets of a run-time MODP group on the GPU (include/mpvss_hip.h, "Key sets of a run-time group"; DESIGN section 13, "Key
sets"): the build, k_rt_keyset_exp through mpvss_modp_group_keyset_dual_exp / _twin_exp, and the two protocol calls that take a
set in place of the key array.

(a) Primitives, per width: a set of 40 keys against Python's pow and, byte for byte, against a2 of group_dleq_commitments and
    group_batch_twin_exp on the same keys.
(b) Protocol: group_deal_keyset and group_verify_distribution_keyset against the plain calls and the oracle's box.
(c) Multi-chunk: a fresh child process per width with MPVSS_MAX_CHUNK=16 (read once per process) runs a box of 45 shares at key
    offset 3.  This file is its own child: `python test_gpu_modp_rt_keyset.py <group>`.
(d) Lifecycle and errors."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_wide_helpers as WH

pytestmark = pytest.mark.gpu

GROUPS = {                                # name -> (q, element bytes, limbs per lane)
    "40": (lambda: H.small_safe_primes()[40], 256, 5),
    "64": (lambda: H.small_safe_primes()[64], 256, 5),
    "256": (lambda: H.small_safe_primes()[256], 256, 5),
    "1024": (lambda: H.rfc_prime(1024), 256, 9),
    "1536": (lambda: H.rfc_prime(1536), 256, 18),
    "2048": (lambda: H.rfc_prime(2048), 256, 18),
    "3072": (WH.group15, WH.EB, 27),
}
NKEYS = 40
SHAPES = [(n, off) for n in (1, 15, 16, 17, 33) for off in (0, 7, 23) if off + n <= NKEYS]


def cat(vals, eb):
    return b"".join(v.to_bytes(eb, "big") for v in vals)


def split(b, eb):
    return [int.from_bytes(b[i:i + eb], "big") for i in range(0, len(b), eb)]


def flip(buf, row, eb, byte=None):
    b = bytearray(buf)
    b[row * eb + (eb - 1 if byte is None else byte)] ^= 1
    return bytes(b)


def make_group(name):
    from mpvss_rs_amd import ModpGroup
    q, eb, lpl = GROUPS[name][0](), GROUPS[name][1], GROUPS[name][2]
    grp = ModpGroup(q, elem_bytes=eb) if eb != 256 else ModpGroup(q)
    assert (grp.elem_bytes, grp.limbs_per_lane) == (eb, lpl)
    return q, eb, grp


def key_values(q, eb, rng):
    """40 keys: 1, q - 1, q (0 mod q), q + 12345, all ones, a duplicate, random units"""
    top = (1 << (8 * eb)) - 1
    keys = [1, q - 1, q, q + 12345, top]
    while len(keys) < NKEYS:
        keys.append(rng.randrange(2, q - 1))
    keys[9] = keys[8]
    return keys


def edge_exponents(q, eb):
    bits, J = 8 * eb, eb // 32
    return ([0, 1, 15, 16, 1 << 255, (1 << 256) - 1, 1 << 256, (1 << 256) + 1] + [1 << (256 * j) for j in range(J)] +
            [9 << (4 * (64 * j + 63)) for j in range(J)] + [1 << (bits - 1), (1 << bits) - 1, q - 1, q - 2])


def e2_values(eb):
    return [0, 1, (1 << 256) - 1, 1 << 256, (1 << (8 * eb)) - 1]


# ---- (a) primitives -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["40", "256", "1024", "1536", "2048", "3072"])
def test_powers_over_a_key_set(engine, name):
    q, eb, grp = make_group(name)
    rng = random.Random(int(name))
    ct = lambda vals: cat(vals, eb)
    sp = lambda b: split(b, eb)
    bits, J = 8 * eb, eb // 32
    keys = key_values(q, eb, rng)
    ks = engine.group_keyset_create(grp, ct(keys))
    try:
        assert ks.nbytes == NKEYS * grp.keyset_bytes_per_key == NKEYS * J * 16 * 4 * grp.limbs_per_lane * 4
        edge, e2v = edge_exponents(q, eb), e2_values(eb)
        g1 = ct([4])

        checked = set()                                                   # edge exponents already compared with pow

        def check(n, off, E1, H2, E2, per_share, rows=()):
            """y^e1 alone, y^e1 h2^e2, and both twin results: byte for byte against the calls that take the keys as bytes, and against
            pow -- the first use of every edge exponent, the five special keys, and all three forms in `rows` (a 3072-bit pow
            takes Python tens of milliseconds, so not every number of every shape)"""
            y = keys[off:off + n]
            alone = engine.group_keyset_dual_exp(grp, ks, off, ct(E1))
            dual = engine.group_keyset_dual_exp(grp, ks, off, ct(E1), ct(H2), ct(E2), per_share)
            Ec = E2 if per_share else E2 * n
            _, a2 = engine.group_dleq_commitments(grp, g1, ct(H2), ct(y), ct(H2), ct(E1), ct(E2), per_share)
            assert dual == a2, (name, n, off)
            T2 = [edge[(3 * i + off) % len(edge)] for i in range(n)]
            twin = engine.group_keyset_twin_exp(grp, ks, off, ct(E1), ct(T2))
            assert twin == engine.group_batch_twin_exp(grp, ct(y), ct(E1), ct(T2)), (name, n, off)
            assert twin[0] == alone
            got, got2, gotd = sp(alone), sp(twin[1]), sp(dual)
            for i in range(n):
                if (E1[i] in edge and E1[i] not in checked) or off + i < 5 or i in rows:
                    checked.add(E1[i])
                    assert got[i] == pow(y[i], E1[i], q), (name, n, off, i)
                if i in rows:
                    assert got2[i] == pow(y[i], T2[i], q), (name, n, off, i)
                    assert gotd[i] == pow(y[i], E1[i], q) * pow(H2[i], Ec[i], q) % q, (name, n, off, i)

        # every shape: the edge exponents in turn; e2 shared (each value in turn) or per share (all values side by side)
        for idx, (n, off) in enumerate(SHAPES):
            E1 = [edge[(i + 5 * idx) % len(edge)] for i in range(n)]
            H2 = [rng.randrange(1 << bits) for _ in range(n)]
            H2[n // 2] = q                                              # h2 = 0 mod q
            per_share = idx % 2 == 1
            E2 = [e2v[(i + idx) % len(e2v)] for i in range(n)] if per_share else [e2v[(idx // 2) % len(e2v)]]
            check(n, off, E1, H2, E2, per_share, rows=(n // 2,))
        assert checked >= set(edge)
        assert {e2v[(idx // 2) % len(e2v)] for idx in range(0, len(SHAPES), 2)} == set(e2v)
        # one wave whose digits are zero in whole rows (the odd ones) and in every third window
        sparse = [sum(rng.randrange(1, 16) << (4 * (64 * j + w)) for j in range(0, J, 2) for w in range(64) if w % 3) for _ in range(16)]
        # one live number among fifteen zeros; short and long exponents side by side
        one_live = [0] * 7 + [rng.getrandbits(bits) | (1 << (bits - 1))] + [0] * 8
        mixed = [rng.getrandbits(64) if i % 2 else rng.getrandbits(bits) | (1 << (bits - 1)) for i in range(16)]
        mixed[3], mixed[4] = rng.getrandbits(300), rng.getrandbits(255)
        for wave, off, rows in ((sparse, 7, (0, 15)), (one_live, 0, (6, 7)), (mixed, 23, (0, 1, 3, 4))):
            check(16, off, wave, [rng.randrange(1 << bits) for _ in range(16)], [rng.getrandbits(256)], False, rows)
        # a second workgroup with 15 dead quads, every exponent of full length
        full = [rng.getrandbits(bits) | (1 << (bits - 1)) for _ in range(17)]
        check(17, 7, full, [rng.randrange(1 << bits) for _ in range(17)], [rng.getrandbits(bits) for _ in range(17)], True, (0, 15, 16))
        # the duplicate key gives the same rows' results
        two = engine.group_keyset_dual_exp(grp, ks, 8, ct([full[0], full[0]]))
        assert two[:eb] == two[eb:]
        # n == 0
        assert engine.group_keyset_dual_exp(grp, ks, NKEYS, b"") == b""
        assert engine.group_keyset_twin_exp(grp, ks, 0, b"", b"") == (b"", b"")
    finally:
        ks.close()


# ---- (b) protocol -----------------------------------------------------------------------------------------------------
_INSTANCES = {}


def instance(name, n, t, seed):
    """a box of the oracle's own dealer over the group, with the randomness kept; computed once and left unchanged"""
    key = (name, n, t, seed)
    if key not in _INSTANCES:
        q = GROUPS[name][0]()
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
        coeffs = [rng.randrange(1, g.q - 1) for _ in range(t)]
        ws = [H.keygen(g, rng) for _ in range(n)]
        box = O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)
        _INSTANCES[key] = (g, pks, coeffs, ws, box)
    return _INSTANCES[key]


def oracle_case(name, n, t, seed):
    q, eb, grp = make_group(name)
    g, pks, coeffs, ws, box = instance(name, n, t, seed)
    keys = [g.element_to_bytes(p) for p in pks]
    return dict(q=q, eb=eb, grp=grp, pks=pks, coeffs=coeffs, ws=ws, box=box, Cm=cat(box["commitments"], eb),
                Y=[box["shares"][k] for k in keys], R=[box["responses"][k] for k in keys], ch=cat([box["challenge"]], eb))


def engine_case(engine, name, n, t, seed):
    """a box dealt by the plain group_deal over random keys (no oracle: a 3072-bit box costs Python many seconds)"""
    q, eb, grp = make_group(name)
    rng = random.Random(seed)
    pks = [rng.randrange(2, q) for _ in range(n)]
    coeffs = [rng.randrange(1, q - 1) for _ in range(t)]
    ws = [rng.randrange(1, q - 1) for _ in range(n)]
    d = engine.group_deal(grp, cat(coeffs, eb), list(range(1, n + 1)), cat(pks, eb), cat(ws, eb))
    Cm = engine.group_batch_exp_fixed_base(grp, cat([4], eb), cat(coeffs, eb))
    return dict(q=q, eb=eb, grp=grp, pks=pks, coeffs=coeffs, ws=ws, box=None, Cm=Cm, Y=split(d["Y"], eb), R=split(d["responses"], eb),
                ch=d["challenge"])


def protocol_checks(engine, name, k, off):
    """both protocol calls over a set that holds the box's keys from key `off` on, against the plain calls and (where the case
    has one) the oracle's box"""
    q, eb, grp, pks, coeffs, ws, box, Cm, Y, R, ch = (k[x] for x in ("q", "eb", "grp", "pks", "coeffs", "ws", "box", "Cm", "Y", "R", "ch"))
    ct = lambda vals: cat(vals, eb)
    sp = lambda b: split(b, eb)
    n = len(pks)
    positions = list(range(1, n + 1))
    front = [5 + i for i in range(off)]
    ks = engine.group_keyset_create(grp, ct(front + pks + [7]))
    bad_row = n - 2
    ks_bad = engine.group_keyset_create(grp, flip(ct(front + pks + [7]), off + bad_row, eb))
    try:
        for mode in (0, 2):                                               # the scalar ring on host threads and on the device
            engine.set_rt_scalar(mode)
            plain = engine.group_deal(grp, ct(coeffs), positions, ct(pks), ct(ws))
            deal = engine.group_deal_keyset(grp, ct(coeffs), positions, ks, off, ct(ws))
            assert deal == plain, (name, mode)
            assert sp(deal["Y"]) == Y and deal["challenge"] == ch and sp(deal["responses"]) == R
            if box:
                assert sp(deal["X"]) == box["_X"] and sp(deal["a1"]) == box["_a1"] and sp(deal["a2"]) == box["_a2"]
                assert deal["digest"] == box["_digest"]
        for mode in (0, 2):                                               # Horner's rule and forward differences for X
            engine.set_rt_fd(mode, 0)
            s0 = engine.group_fd_stats()
            v = engine.group_verify_distribution_keyset(grp, Cm, positions, ks, off, ct(Y), ct(R), ch, dump=True)
            s1 = engine.group_fd_stats()
            chunks = -(-n // int(os.environ.get("MPVSS_MAX_CHUNK", 1 << 18)))
            assert (s1["fd"] - s0["fd"], s1["horner"] - s0["horner"]) == ((chunks, 0) if mode == 2 else (0, chunks))
            assert v == engine.group_verify_distribution(grp, Cm, positions, ct(pks), ct(Y), ct(R), ch, dump=True)
            assert v["verdict"] is True and v["digest"] == deal["digest"]
            assert v["X"] == deal["X"] and v["a1"] == deal["a1"] and v["a2"] == deal["a2"]
            assert engine.group_verify_distribution_keyset(grp, Cm, positions, ks, off, ct(Y), ct(R), ch) == \
                {"verdict": True, "digest": deal["digest"]}                       # without the dumps
            for shares, resp in ((ct(Y), flip(ct(R), bad_row, eb)), (flip(ct(Y), bad_row, eb), ct(R))):
                bad = engine.group_verify_distribution_keyset(grp, Cm, positions, ks, off, shares, resp, ch, dump=True)
                assert bad["verdict"] is False
                assert bad == engine.group_verify_distribution(grp, Cm, positions, ct(pks), shares, resp, ch, dump=True)
            bad = engine.group_verify_distribution_keyset(grp, Cm, positions, ks_bad, off, ct(Y), ct(R), ch, dump=True)
            assert bad["verdict"] is False and bad["a2"] != v["a2"] and bad["a1"] == v["a1"]
            assert bad == engine.group_verify_distribution(grp, Cm, positions, flip(ct(pks), bad_row, eb), ct(Y), ct(R), ch, dump=True)
            # a caller's challenge as long as the element: the exponent of Y has more than 64 windows
            long_c = ct([random.Random(n).getrandbits(8 * eb) | (1 << (8 * eb - 1))])
            lv = engine.group_verify_distribution_keyset(grp, Cm, positions, ks, off, ct(Y), ct(R), long_c, dump=True)
            assert lv == engine.group_verify_distribution(grp, Cm, positions, ct(pks), ct(Y), ct(R), long_c, dump=True)
            assert lv["verdict"] is False and lv["a2"] != v["a2"]
    finally:
        engine.set_rt_scalar(1)
        engine.set_rt_fd(1, 0)
        ks.close()
        ks_bad.close()


@pytest.mark.parametrize("n,t", [(17, 5), (33, 4)])
@pytest.mark.parametrize("name", ["256", "1024", "2048", "3072"])
def test_protocol_calls_over_a_key_set(engine, name, n, t):
    protocol_checks(engine, name, oracle_case(name, n, t, 31), off=2 if n == 17 else 0)


def test_the_callers_2048_bit_challenge(engine):
    """the 2048-bit group with a challenge of exactly 2048 bits on both paths (protocol_checks runs one per width too)"""
    q, eb, grp = make_group("2048")
    g, pks, coeffs, ws, box = instance("2048", 17, 5, 31)
    keys = [g.element_to_bytes(p) for p in pks]
    ct = lambda vals: cat(vals, eb)
    Y, R = [box["shares"][k] for k in keys], [box["responses"][k] for k in keys]
    c = ct([(1 << 2047) | random.Random(2).getrandbits(2047)])
    with engine.group_keyset_create(grp, ct(pks)) as ks:
        got = engine.group_verify_distribution_keyset(grp, ct(box["commitments"]), list(range(1, 18)), ks, 0, ct(Y), ct(R), c, dump=True)
    want = engine.group_verify_distribution(grp, ct(box["commitments"]), list(range(1, 18)), ct(pks), ct(Y), ct(R), c, dump=True)
    assert got == want and got["verdict"] is False
    c_int = int.from_bytes(c, "big")
    assert split(got["a2"], eb) == [pow(y, r, q) * pow(s, c_int, q) % q for y, s, r in zip(pks, Y, R)]


# ---- (c) the child: several chunks --------------------------------------------------------------------------------------
N, T, CHUNK, OFF = 45, 3, 16, 3


def child(name):
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(CHUNK)
    eng = Engine(0)
    k = engine_case(eng, name, N, T, seed=7)
    protocol_checks(eng, name, k, OFF)                                  # the set's 49 keys are built in chunks too
    q, eb, grp, pks, ws = k["q"], k["eb"], k["grp"], k["pks"], k["ws"]
    rng = random.Random(5)
    e1 = [rng.getrandbits(8 * eb) for _ in range(N)]
    e2 = [rng.randrange(q) for _ in range(N)]
    with eng.group_keyset_create(grp, cat([5, 6, 7] + pks, eb)) as ks:
        assert eng.group_keyset_twin_exp(grp, ks, OFF, cat(e1, eb), cat(e2, eb)) == eng.group_batch_twin_exp(grp, cat(pks, eb), cat(e1, eb), cat(e2, eb))
        got = eng.group_keyset_dual_exp(grp, ks, OFF, cat(e1, eb), cat(ws, eb), cat(e2, eb), True)
        assert got == eng.group_dleq_commitments(grp, cat([4], eb), cat(ws, eb), cat(pks, eb), cat(ws, eb), cat(e1, eb), cat(e2, eb), True)[1]
        for i in (0, 15, 16, 31, 32, 44):                               # the edges of the three chunks against pow
            assert split(got, eb)[i] == pow(pks[i], e1[i], q) * pow(ws[i], e2[i], q) % q
    eng.close()
    print("keyset child ok")


def test_multi_chunk_calls_in_a_fresh_process_per_group():
    """one child after another, stopping at the first that fails"""
    for name, timeout in (("64", 120), ("1024", 120), ("2048", 180), ("3072", 240)):
        env = dict(os.environ, MPVSS_MAX_CHUNK=str(CHUNK))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, env=env, timeout=timeout)
        assert out.returncode == 0, f"group {name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
        assert "keyset child ok" in out.stdout


# ---- (d) lifecycle and errors -------------------------------------------------------------------------------------------
def test_two_sets_and_four_threads(engine):
    q, eb, grp = make_group("1024")
    rng = random.Random(4)
    A = [rng.randrange(2, q) for _ in range(20)]
    B = [rng.randrange(2, q) for _ in range(9)]
    ksA, ksB = engine.group_keyset_create(grp, cat(A, eb)), engine.group_keyset_create(grp, cat(B, eb))
    try:
        jobs = [(off, [rng.getrandbits(1024) for _ in range(20 - off)]) for off in (0, 3, 11, 19)]
        want = [[pow(b, e, q) for b, e in zip(A[off:], E)] for off, E in jobs]
        eB = [rng.getrandbits(1024) for _ in B]
        assert split(engine.group_keyset_dual_exp(grp, ksB, 0, cat(eB, eb)), eb) == [pow(b, e, q) for b, e in zip(B, eB)]
        got, errors = [None] * 4, []

        def work(i):
            try:
                for _ in range(3):
                    got[i] = split(engine.group_keyset_dual_exp(grp, ksA, jobs[i][0], cat(jobs[i][1], eb)), eb)
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors and got == want
        assert split(engine.group_keyset_dual_exp(grp, ksB, 0, cat(eB, eb)), eb) == [pow(b, e, q) for b, e in zip(B, eB)]
    finally:
        ksA.close()
        ksB.close()


def test_refusals_leave_the_context_working(engine):
    from mpvss_rs_amd import Engine, EngineError, ModpGroup
    q, eb, grp = make_group("256")
    other = ModpGroup(H.small_safe_primes()[128])                       # the same width, another modulus
    wide = make_group("3072")[2]
    keys = [3, 5, 7, 11]
    ks = engine.group_keyset_create(grp, cat(keys, eb))
    e = cat([2, 3, 4, 5], eb)
    works = lambda: split(engine.group_keyset_dual_exp(grp, ks, 0, e), eb) == [9, 125, 2401, 161051 % q]
    try:
        assert works()
        second = Engine(0)
        try:
            with pytest.raises(EngineError, match="rc=-1"):                 # a set of another context
                second.group_keyset_dual_exp(grp, ks, 0, e)
            with pytest.raises(EngineError, match="rc=-1"):
                second.group_deal_keyset(grp, cat([1, 2], eb), [1, 2, 3, 4], ks, 0, e)
        finally:
            second.close()
        assert works()
        for g2 in (other, wide):                                         # a handle of another modulus / another width
            with pytest.raises(EngineError, match="rc=-1"):
                engine.group_keyset_twin_exp(g2, ks, 0, cat([2], g2.elem_bytes), cat([3], g2.elem_bytes))
            assert works()
        for off, n in ((1, 4), (4, 1), (5, 0), (2 ** 63, 2 ** 63)):      # key_offset + n past the end (and wrapping around)
            with pytest.raises(EngineError, match="rc=-1"):
                engine.group_keyset_dual_exp(grp, ks, off, cat([2] * min(n, 4), eb)) if n <= 4 else \
                    engine._check(engine.lib.mpvss_modp_group_keyset_dual_exp(engine.ctx, grp.handle, 0, ks.handle, off, e, None, None, 0,
                                                                              n, e), "group_keyset_dual_exp")
            assert works()
        with pytest.raises(EngineError, match="rc=-1"):
            engine.group_verify_distribution_keyset(grp, e, [1, 2, 3, 4], ks, 1, e, e, cat([1], eb))
        with pytest.raises(EngineError, match="rc=-1"):                     # no set at all
            engine._check(engine.lib.mpvss_modp_group_keyset_dual_exp(engine.ctx, grp.handle, 0, None, 0, e, None, None, 0, 4, e), "x")
        with pytest.raises(EngineError, match="rc=-1"):                     # no group under a live context
            engine._check(engine.lib.mpvss_modp_group_keyset_dual_exp(engine.ctx, None, 0, ks.handle, 0, e, None, None, 0, 4, e), "x")
        h = C.c_void_p(1)
        assert engine.lib.mpvss_modp_group_keyset_create(engine.ctx, None, 0, e, 4, C.byref(h)) == -1 and h.value is None
        with pytest.raises(EngineError, match="rc=-1"):                     # create: n == 0, a null pointer
            engine.group_keyset_create(grp, b"")
        assert engine.lib.mpvss_modp_group_keyset_create(engine.ctx, grp.handle, 0, None, 4, C.byref(h)) == -1
        assert engine.lib.mpvss_modp_group_keyset_create(engine.ctx, grp.handle, 0, e, 4, None) == -1
        assert works()
        # the empty box: the digest of the empty transcript on both paths
        d = hashlib.sha256(b"").digest()
        assert engine.group_deal_keyset(grp, b"", [], ks, 0, b"") == engine.group_deal(grp, b"", [], b"", b"")
        ch = engine.group_deal(grp, b"", [], b"", b"")["challenge"]
        v = engine.group_verify_distribution_keyset(grp, b"", [], ks, 4, b"", b"", ch)
        assert v == engine.group_verify_distribution(grp, b"", [], b"", b"", b"", ch) and v == {"verdict": True, "digest": d}
    finally:
        ks.close()
    # destroy, then create again
    ks = engine.group_keyset_create(grp, cat(keys, eb))
    assert works()
    ks.close()
    ks.close()


def test_device_space_keys_equal_host_keys(engine):
    import torch
    q, eb, grp = make_group("2048")
    rng = random.Random(8)
    keys = [rng.randrange(1 << 2048) for _ in range(19)]
    E = [rng.getrandbits(2048) for _ in keys]
    dev = torch.frombuffer(bytearray(cat(keys, eb)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with engine.group_keyset_create_device(grp, dev.data_ptr(), len(keys)) as kd, engine.group_keyset_create(grp, cat(keys, eb)) as kh:
        assert kd.nbytes == kh.nbytes == 19 * 36864
        got = engine.group_keyset_dual_exp(grp, kd, 0, cat(E, eb))
        assert got == engine.group_keyset_dual_exp(grp, kh, 0, cat(E, eb))
        assert split(got, eb) == [pow(b, e, q) for b, e in zip(keys, E)]
        # results in device space equal results in host space
        e_dev = torch.frombuffer(bytearray(cat(E, eb)), dtype=torch.uint8).cuda()
        o1 = torch.zeros(19 * eb, dtype=torch.uint8, device="cuda")
        o2 = torch.zeros(19 * eb, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert engine.lib.mpvss_modp_group_keyset_twin_exp(engine.ctx, grp.handle, 1, kd.handle, 0, C.c_void_p(e_dev.data_ptr()),
                                                           C.c_void_p(e_dev.data_ptr()), 19, C.c_void_p(o1.data_ptr()),
                                                           C.c_void_p(o2.data_ptr())) == 0
        assert bytes(o1.cpu().numpy()) == got == bytes(o2.cpu().numpy())


def test_timers_cover_the_build_and_the_launches(engine):
    q, eb, grp = make_group("1024")
    keys = [random.Random(1).randrange(q) for _ in range(16)]
    ks = engine.group_keyset_create(grp, cat(keys, eb))
    try:
        assert [engine.kernel_launches(i) for i in range(5)] == [0, 0, 1, 0, 0] and engine.kernel_ms(2) > 0      # the build: timer 2
        engine.group_keyset_dual_exp(grp, ks, 0, cat(keys, eb))
        assert [engine.kernel_launches(i) for i in range(5)] == [0, 0, 0, 1, 0] and engine.kernel_ms(3) > 0      # the launch: timer 3
        engine.group_keyset_dual_exp(grp, ks, 0, cat(keys, eb), cat(keys, eb), cat([5], eb))
        assert [engine.kernel_launches(i) for i in range(5)] == [0, 0, 1, 1, 0]                                  # and h2's tables
        engine.group_keyset_twin_exp(grp, ks, 0, cat(keys, eb), cat(keys, eb))
        assert [engine.kernel_launches(i) for i in range(5)] == [0, 0, 0, 1, 0]
    finally:
        ks.close()


if __name__ == "__main__":
    child(sys.argv[1])
