"""The row layout for small calls of a run-time MODP group (mpvss_ctx_set_rt_row; modp_rt_row_kernels.hip: 16 lanes per number) on
handles for RFC 3526 groups 14, 15 and 16 (18 / 27 / 36 limbs per lane) and on one 1024-bit handle (9 limbs per lane: no row
layout).  Every comparison is mode 2 against mode 0 on the same context, byte for byte, and against Python's pow on a sample;
mpvss_modp_group_row_stats says which layout the launches took."""
import functools
import random

import pytest

import modp_rt_helpers as H
import modp_rt_many_helpers as MH
import modp_rt_wide_helpers as WH
import modp_rt_4096_helpers as XH
from mpvss_rs_amd import Engine, ModpGroup, capi

pytestmark = pytest.mark.gpu

GROUPS = {                                   # name -> (q, element bytes, limbs per lane)
    "14": (lambda: H.rfc_prime(2048), 256, 18),
    "15": (WH.group15, 384, 27),
    "16": (XH.group16, 512, 36),
    "1024": (lambda: H.rfc_prime(1024), 256, 9),
}
WIDE = ("14", "15", "16")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def handles():
    hs = {}
    for name, (q, eb, lpl) in GROUPS.items():
        g = ModpGroup(q(), elem_bytes=eb) if eb != 256 else ModpGroup(q())
        assert (g.elem_bytes, g.limbs_per_lane) == (eb, lpl)
        hs[name] = g
    yield hs
    for g in hs.values():
        g.close()


def cat(vals, eb):
    return b"".join(v.to_bytes(eb, "big") for v in vals)


def split(b, eb):
    return [int.from_bytes(b[i:i + eb], "big") for i in range(0, len(b), eb)]


def both(eng, name, call, launches=None):
    """call() under mode 0 and under mode 2 on the same context: equal results; no row launch under mode 0; under mode 2 no quad
    launch on a wide handle (and `launches` row launches when given), no row launch on the 1024-bit one.  Returns the result."""
    assert eng.set_rt_row(0) in (0, 1, 2)
    s0 = eng.group_row_stats()
    a = call()
    s1 = eng.group_row_stats()
    assert eng.set_rt_row(2) == 0
    b = call()
    s2 = eng.group_row_stats()
    assert eng.set_rt_row(0) == 2
    assert a == b
    assert s1["row"] == s0["row"] and s1["quad"] > s0["quad"]
    if name in WIDE:
        assert s2["quad"] == s1["quad"] and s2["row"] - s1["row"] == s1["quad"] - s0["quad"]
    else:
        assert s2["row"] == s1["row"] and s2["quad"] - s1["quad"] == s1["quad"] - s0["quad"]
    if launches is not None:
        assert s1["quad"] - s0["quad"] == launches
    return a


@functools.lru_cache(maxsize=None)
def exp_rows(name):
    """17 (base, exponent, pow) rows of a group, computed once: wave 0 the named edges, wave 1 four exponents that are all 0, wave 2
    a 3-bit exponent beside a full-width one, wave 3 more edges, and a ragged last wave"""
    q, eb, _ = GROUPS[name]
    q = q()
    rng = random.Random(eb + q % 1000)
    ones = (1 << (8 * eb)) - 1                          # EB bytes of ones: longer than q
    e0f, ef0 = int("0f" * eb, 16), int("f0" * eb, 16)
    rnd = lambda: rng.randrange(2, q)
    rows = [(0, q - 2), (1, ones), (q - 1, q - 2), (q + 5, e0f),
            (rnd(), 0), (rnd(), 0), (q - 1, 0), (0, 0),
            (rnd(), 5), (rnd(), ones), (rnd(), 1), (0, 0),
            (rnd(), ef0), (q - 1, 1), (rnd(), 0), (1, 0),
            (rnd(), q - 2)]
    return [(b, e, pow(b, e, q)) for b, e in rows]


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_batch_exp_under_both_modes(eng, handles, name):
    grp, eb = handles[name], GROUPS[name][1]
    rows = exp_rows(name)
    for sel in (rows[16:], rows[:5], rows):               # n = 1, 5, 17
        B, E, want = zip(*sel)
        out = both(eng, name, lambda: eng.group_batch_exp(grp, cat(B, eb), cat(E, eb)), launches=1)
        assert split(out, eb) == list(want), len(sel)


def test_batch_exp_at_4096_and_4097_numbers_and_the_automatic_mode(eng, handles):
    """2048 bits: 4096 numbers are one wave per SIMD on the row layout, 4097 have a ragged last wave; mode 1 takes the row layout
    at 4096 numbers and the quad layout at 4097, and the first 4096 results are equal"""
    grp, q, eb = handles["14"], H.rfc_prime(2048), 256
    assert eng.group_row_max_shares(grp) == 4096
    rng = random.Random(4097)
    n = 4097
    B = [rng.randrange(2, q) for _ in range(n)]
    E = [rng.getrandbits(2048) for _ in range(n)]
    E[4096], E[4095], E[7] = (1 << 2048) - 1, 0, 3
    cb, ce = cat(B, eb), cat(E, eb)
    full = both(eng, "14", lambda: eng.group_batch_exp(grp, cb, ce), launches=1)
    part = both(eng, "14", lambda: eng.group_batch_exp(grp, cb[:4096 * eb], ce[:4096 * eb]), launches=1)
    assert full[:4096 * eb] == part
    got = split(full, eb)
    for i in (0, 7, 4095, 4096):
        assert got[i] == pow(B[i], E[i], q), i
    assert eng.set_rt_row(1) == 0
    try:
        s0 = eng.group_row_stats()
        auto_part = eng.group_batch_exp(grp, cb[:4096 * eb], ce[:4096 * eb])
        s1 = eng.group_row_stats()
        auto_full = eng.group_batch_exp(grp, cb, ce)
        s2 = eng.group_row_stats()
    finally:
        assert eng.set_rt_row(0) == 1
    assert (s1["row"] - s0["row"], s1["quad"] - s0["quad"]) == (1, 0)
    assert (s2["row"] - s1["row"], s2["quad"] - s1["quad"]) == (0, 1)
    assert auto_part == part and auto_full == full


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_dleq_commitments_under_both_modes(eng, handles, name):
    """n = 37; a non-generator g1 goes through a shared table of stride 0; c shared, per share, and longer than 256 bits; once
    after group_prepare with g1 = g = 4, so that a1 runs over the comb"""
    grp, eb = handles[name], GROUPS[name][1]
    q = GROUPS[name][0]()
    rng = random.Random(37 + eb)
    n = 37
    h1, g2, h2 = ([rng.randrange(2, q) for _ in range(n)] for _ in range(3))
    r = [rng.randrange(q - 1) for _ in range(n)]
    r[0], r[1], r[2] = 0, q - 2, 1
    flat = lambda xs: cat(xs, eb)

    def check(g1, cs, per, sample):
        a1, a2 = both(eng, name, lambda: eng.group_dleq_commitments(grp, cat([g1], eb), flat(h1), flat(g2), flat(h2), flat(r),
                                                                     flat(cs) if per else cat([cs[0]], eb), per), launches=2)
        A1, A2 = split(a1, eb), split(a2, eb)
        for i in sample:
            assert A1[i] == pow(g1, r[i], q) * pow(h1[i], cs[i], q) % q, i
            assert A2[i] == pow(g2[i], r[i], q) * pow(h2[i], cs[i], q) % q, i

    per_share = [rng.getrandbits(256) for _ in range(n)]
    per_share[0] = 0
    check(7, per_share, True, (0, 1, 36))
    check(7, [rng.getrandbits(256)] * n, False, (2,))
    check(7, [(1 << 300) + 77] * n, False, (36,))
    before = eng.group_comb_stats()
    eng.group_prepare(grp)
    check(4, [rng.getrandbits(256)] * n, False, (1, 35))
    assert eng.group_comb_stats()["hits"] - before["hits"] >= 2       # a1 went over the comb under both modes


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_twin_exp_and_fixed_base_under_both_modes(eng, handles, name):
    grp, eb = handles[name], GROUPS[name][1]
    q = GROUPS[name][0]()
    rng = random.Random(9 + eb)
    rows = exp_rows(name)
    B = [b for b, _, _ in rows[8:17]]                       # n = 9: two exponent sets over one table
    E1 = [e for _, e, _ in rows[8:17]]
    E2 = [rng.getrandbits(64), 0, (1 << (8 * eb)) - 1, 1, 2, rng.getrandbits(8 * eb), 0, 15, 16]
    assert len(B) < grp.twin_min_shares
    o1, o2 = both(eng, name, lambda: eng.group_batch_twin_exp(grp, cat(B, eb), cat(E1, eb), cat(E2, eb)), launches=1)
    assert split(o1, eb) == [w for _, _, w in rows[8:17]]
    got2 = split(o2, eb)
    for i in (0, 1, 3, 4, 5, 8):
        assert got2[i] == pow(B[i], E2[i], q), i
    # a fixed base the context has no comb of, n = 6: one shared table
    base = rows[8][0]
    E = [rows[8][1], rows[9][1], 0, 1, rng.getrandbits(100), q - 2]
    assert len(E) < grp.comb_min_shares
    out = both(eng, name, lambda: eng.group_batch_exp_fixed_base(grp, cat([base], eb), cat(E, eb)), launches=1)
    got = split(out, eb)
    assert got[0] == rows[8][2] and got[2] == 1 and got[3] == base
    assert got[4] == pow(base, E[4], q)


def _flip(buf, row, eb, byte=None):
    b = bytearray(buf)
    b[row * eb + (eb - 1 if byte is None else byte)] ^= 1
    return bytes(b)


def _keys(eng, grp, q, eb, n, rng):
    """n private keys coprime to q - 1 = 2 q' (odd, not q'), their inverses mod q - 1, and the public keys G^x"""
    privs = []
    while len(privs) < n:
        k = rng.randrange(3, q - 1) | 1
        if k != (q - 1) // 2:
            privs.append(k)
    pks = eng.group_batch_exp_fixed_base(grp, cat([2], eb), cat(privs, eb))
    return privs, [pow(k, -1, q - 1) for k in privs], pks


@pytest.mark.parametrize("name", WIDE)
def test_one_protocol_run_per_width(eng, handles, name):
    """(n, t) = (5, 3): deal -> verify_distribution (verdict 1, the dealer's digest reproduced) -> extract_shares -> verify_shares ->
    reconstruct (once with the Lagrange exponents on the device): every output equal under modes 0 and 2, G^s = G^(a_0), and a
    flipped response bit rejected under mode 2"""
    grp, eb = handles[name], GROUPS[name][1]
    q = GROUPS[name][0]()
    rng = random.Random(53 + eb)
    n, t = 5, 3
    positions = list(range(1, n + 1))
    privs, xinv, pks = _keys(eng, grp, q, eb, n, rng)
    coeffs = [rng.randrange(1, q - 1) for _ in range(t)]
    ws, w2 = [rng.randrange(1, q - 1) for _ in range(n)], [rng.randrange(1, q - 1) for _ in range(n)]
    C = eng.group_batch_exp_fixed_base(grp, cat([4], eb), cat(coeffs, eb))
    box = both(eng, name, lambda: eng.group_deal(grp, cat(coeffs, eb), positions, pks, cat(ws, eb)))
    v = both(eng, name, lambda: eng.group_verify_distribution(grp, C, positions, pks, box["Y"], box["responses"], box["challenge"],
                                                              dump=True))
    assert v["verdict"] is True and v["digest"] == box["digest"]
    assert (v["X"], v["a1"], v["a2"]) == (box["X"], box["a1"], box["a2"])
    S, Cs = both(eng, name, lambda: eng.group_extract_shares(grp, pks, box["Y"], cat(xinv, eb), cat(w2, eb)))
    P1 = sum(c * 1 ** j for j, c in enumerate(coeffs)) % (q - 1)
    assert split(S, eb)[0] == pow(2, P1, q)                                   # S_1 = G^P(1)
    R = capi.group_dleq_responses(grp, cat(w2, eb), cat(privs, eb), Cs)
    ok = both(eng, name, lambda: bytes(eng.group_verify_shares(grp, pks, S, box["Y"], Cs, R)))
    assert list(ok) == [1] * n
    pick = [0, 2, 4]
    sub = b"".join(S[i * eb:(i + 1) * eb] for i in pick)
    gs, mask = both(eng, name, lambda: eng.group_reconstruct(grp, [positions[i] for i in pick], sub))
    assert int.from_bytes(gs, "big") == pow(2, coeffs[0], q)
    before = eng.set_rt_lagrange(2)
    try:
        assert both(eng, name, lambda: eng.group_reconstruct(grp, [positions[i] for i in pick], sub)) == (gs, mask)
    finally:
        eng.set_rt_lagrange(before)
    assert eng.set_rt_row(2) == 0
    try:
        bad = eng.group_verify_distribution(grp, C, positions, pks, box["Y"], _flip(box["responses"], n - 1, eb), box["challenge"])
        bad_s = list(eng.group_verify_shares(grp, pks, S, box["Y"], Cs, _flip(R, 1, eb, 200 % eb)))
    finally:
        assert eng.set_rt_row(0) == 2
    assert bad["verdict"] is False
    assert bad_s == [1, 0, 1, 1, 1]


def test_verify_many_and_reconstruct_many_at_2048_bits(eng, handles):
    """seven boxes of modp_rt_many_helpers.SHAPES in one group_verify_many call (one of them with a flipped share) and five secrets in
    one group_reconstruct_many call: the same verdicts, digests, G^s and masks under modes 0 and 2"""
    grp, q, eb = handles["14"], H.rfc_prime(2048), 256
    rng = random.Random(77)
    boxes, digests = [], []
    for n, t in MH.SHAPES:
        positions = list(range(1, n + 1))
        _, _, pks = _keys(eng, grp, q, eb, n, rng)
        coeffs = [rng.randrange(1, q - 1) for _ in range(t)]
        d = eng.group_deal(grp, cat(coeffs, eb), positions, pks, cat([rng.randrange(1, q - 1) for _ in range(n)], eb))
        boxes.append(dict(commitments=eng.group_batch_exp_fixed_base(grp, cat([4], eb), cat(coeffs, eb)), positions=positions,
                          pubkeys=pks, shares=d["Y"], responses=d["responses"], challenge=d["challenge"]))
        digests.append(d["digest"])
    boxes[3] = dict(boxes[3], shares=_flip(boxes[3]["shares"], 5, eb))
    got = both(eng, "14", lambda: eng.group_verify_many(grp, boxes))
    assert [v for v, _ in got] == [i != 3 for i in range(len(boxes))]
    assert [d for i, (_, d) in enumerate(got) if i != 3] == [d for i, d in enumerate(digests) if i != 3]
    # five secrets: the shares S_i = G^P(i) of one polynomial at five position lists of three
    n, t = 5, 3
    coeffs = [rng.randrange(1, q - 1) for _ in range(t)]
    P = [sum(c * i ** j for j, c in enumerate(coeffs)) % (q - 1) for i in range(1, n + 1)]
    S = eng.group_batch_exp_fixed_base(grp, cat([2], eb), cat(P, eb))
    picks = [(0, 1, 2), (2, 3, 4), (0, 2, 4), (1, 3, 4), (4, 0, 1)]
    secrets = [dict(positions=[i + 1 for i in pick], shares=b"".join(S[i * eb:(i + 1) * eb] for i in pick)) for pick in picks]
    rec = both(eng, "14", lambda: eng.group_reconstruct_many(grp, secrets))
    assert [s for s, _, _ in rec] == [0] * 5
    assert {int.from_bytes(gs, "big") for _, gs, _ in rec} == {pow(2, coeffs[0], q)}
    assert len({m for _, _, m in rec}) == 1


def test_the_setter_the_bound_and_the_counters(eng, handles):
    assert eng.set_rt_row(0) == 0                                               # the default
    assert [eng.group_row_max_shares(handles[k]) for k in ("14", "15", "16", "1024")] == [4096, 4096, 4096, 0]
    assert eng.lib.mpvss_modp_group_row_max_shares(None) == 0
    assert eng.set_rt_row(1) == 0 and eng.set_rt_row(2) == 1 and eng.set_rt_row(0) == 2
    assert eng.lib.mpvss_ctx_set_rt_row(eng.ctx, 3) < 0 and eng.lib.mpvss_ctx_set_rt_row(eng.ctx, -1) < 0
    assert eng.set_rt_row(0) == 0                                               # a refused value leaves the mode
    assert eng.lib.mpvss_ctx_set_rt_row(None, 1) < 0
    assert eng.lib.mpvss_modp_group_row_stats(None, None, None) < 0
    assert eng.lib.mpvss_modp_group_row_stats(eng.ctx, None, None) == 0
    # mode 1 on the 1024-bit handle: the quad layout, the bytes of mode 0
    grp, q, eb = handles["1024"], H.rfc_prime(1024), 256
    B, E = [3, q - 1, 5], [q - 2, 7, (1 << 2048) - 1]
    want = eng.group_batch_exp(grp, cat(B, eb), cat(E, eb))
    assert eng.set_rt_row(1) == 0
    try:
        s0 = eng.group_row_stats()
        assert eng.group_batch_exp(grp, cat(B, eb), cat(E, eb)) == want
        s1 = eng.group_row_stats()
    finally:
        assert eng.set_rt_row(0) == 1
    assert (s1["row"] - s0["row"], s1["quad"] - s0["quad"]) == (0, 1)
    assert split(want, eb) == [pow(b, e, q) for b, e in zip(B, E)]
