"""The scalar ring Z/(q-1) of a run-time MODP group on the device: mpvss_modp_group_batch_scalar_mul, _dleq_responses_device and
_poly_eval_device against the host entry points of the same handle (which tests/test_modp_rt_scalar_host.py holds to Python
integers), and group_deal / group_extract_shares under mpvss_ctx_set_rt_scalar mode 0 and mode 2 against each other and the
oracle.  Exact integers everywhere: every comparison is of bytes.  One modulus per width (5, 5, 9, 18, 27 limbs per lane); n = 1,
15, 16, 17, 33 straddles one and two 16-number workgroups and exercises the clamped tail quads."""
import functools
import random

import pytest
import torch

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
from mpvss_rs_amd import ModpGroup, capi
from mpvss_rs_amd.capi import EngineError

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 33)


def _groups():
    sp = H.small_safe_primes()
    return [(23, 256), (sp[512], 256), (H.rfc_prime(1024), 256), (H.rfc_prime(2048), 256), (WH.group15(), 384)]


GROUPS = _groups()
IDS = [f"{q.bit_length()}b" for q, _ in GROUPS]
_cache = {}


def handle(q, eb):
    if q not in _cache:
        _cache[q] = ModpGroup(q) if eb == 256 else ModpGroup(q, elem_bytes=eb)
    return _cache[q]


def cat(vals, eb):
    return b"".join(v.to_bytes(eb, "big") for v in vals)


def dev_u8(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")


def edge(q, eb):
    qh = (q - 1) // 2
    return [0, 1, qh - 1, qh, q - 2, q - 1, q, (1 << (8 * eb)) - 1]


def operands(q, eb, n, rng, shift):
    """n operands: the eight edge values (at n < 8, the n that follow edge number `shift`), then random reduced and unreduced ones,
    rotated to the right by `shift` rows.  Over shift = 0 .. max(n, 8) - 1 (`shifts`) every edge value meets every row position,
    those of the last partial wave included: row p holds element (p - shift) mod n of the list."""
    e = edge(q, eb)
    out = list(e) if n >= len(e) else [e[(shift + i) % len(e)] for i in range(n)]
    while len(out) < n:
        out.append(rng.randrange(q) if len(out) % 2 else rng.randrange(1 << (8 * eb)))
    k = shift % n
    return out[n - k:] + out[:n - k]


def shifts(n):
    return range(max(n, 8))


def test_operands_put_every_edge_value_in_every_row():
    q, eb = 23, 256
    rng = random.Random(0)
    for n in NS:
        for offset in (0, 5):
            seen = {(p, v) for s in shifts(n) for p, v in enumerate(operands(q, eb, n, rng, s + offset))}
            assert all((p, v) in seen for p in range(n) for v in edge(q, eb)), (n, offset)


@pytest.fixture(autouse=True)
def _default_mode(engine):
    engine.set_rt_scalar(1)
    yield
    engine.set_rt_scalar(1)


@pytest.mark.parametrize("q,eb", GROUPS, ids=IDS)
def test_batch_scalar_mul_both_spaces(engine, q, eb):
    grp = handle(q, eb)
    rng = random.Random(q & 0xFFFF)
    for n in NS:
        for shift in shifts(n):
            a = operands(q, eb, n, rng, shift)
            b = operands(q, eb, n, rng, shift + 5)
            want = b"".join(capi.group_scalar_mul(grp, x.to_bytes(eb, "big"), y.to_bytes(eb, "big")) for x, y in zip(a, b))
            assert engine.group_batch_scalar_mul(grp, cat(a, eb), cat(b, eb)) == want, (n, shift)
            da, db = dev_u8(cat(a, eb)), dev_u8(cat(b, eb))
            out = torch.full((n * eb + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            engine.group_batch_scalar_mul_device(grp, da.data_ptr(), db.data_ptr(), n, out.data_ptr())
            raw = out.cpu().numpy().tobytes()
            assert raw[: n * eb] == want and raw[n * eb:] == b"\xa5" * 64, (n, shift)


@pytest.mark.parametrize("q,eb", GROUPS, ids=IDS)
def test_dleq_responses_device(engine, q, eb):
    grp = handle(q, eb)
    rng = random.Random(q & 0xFFFFF)
    qh = (q - 1) // 2
    for ci, c in enumerate((0, qh, q - 2, rng.randrange(1 << (8 * eb)))):
        for n, shift in ((n, s) for n in NS for s in shifts(n)):
            w = operands(q, eb, n, rng, shift)
            alpha = operands(q, eb, n, rng, shift + 3)
            want = capi.group_dleq_responses(grp, cat(w, eb), cat(alpha, eb), c.to_bytes(eb, "big"), threads=1)
            dw, da = dev_u8(cat(w, eb)), dev_u8(cat(alpha, eb))
            out = torch.full((n * eb + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            engine.group_dleq_responses_device(grp, dw.data_ptr(), da.data_ptr(), c.to_bytes(eb, "big"), n, out.data_ptr())
            raw = out.cpu().numpy().tobytes()
            assert raw[: n * eb] == want and raw[n * eb:] == b"\x5a" * 64, (c, n, shift)


def _poly_device(engine, grp, eb, coeffs, positions):
    n = len(positions)
    d_pos = torch.tensor(positions, dtype=torch.int64, device="cuda:0")
    out = torch.full((n * eb + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.group_poly_eval_device(grp, cat(coeffs, eb), d_pos.data_ptr(), n, out.data_ptr())
    raw = out.cpu().numpy().tobytes()
    assert raw[n * eb:] == b"\xa5" * 64
    return raw[: n * eb]


@pytest.mark.parametrize("q,eb", GROUPS, ids=IDS)
@pytest.mark.parametrize("t", [1, 2, 3, 17])
def test_poly_eval_device(engine, q, eb, t):
    grp = handle(q, eb)
    rng = random.Random(t * 977 + (q & 0xFFF))
    e = edge(q, eb)
    coeffs = [rng.randrange(q - 1) for _ in range(t)]
    for k, v in enumerate((0, q - 2, q - 1, (1 << (8 * eb)) - 1, q)):           # 0, q - 2 and values >= q - 1
        if k < t:
            coeffs[(k * 5) % t] = v
    special = [0, 1, 2, 1 << 31, (1 << 63) - 1]
    for n in NS:
        positions = (special + list(range(7, 7 + 40)))[:n] if n != 16 else list(range(1, 17))
        if n == 33:
            positions = special + list(range((1 << 31) - 14, (1 << 31) + 14))
        want = capi.group_poly_eval(grp, cat(coeffs, eb), positions, threads=1)
        assert _poly_device(engine, grp, eb, coeffs, positions) == want, (t, n)
    # all-edge coefficients
    coeffs = [e[(j * 3 + t) % len(e)] for j in range(t)]
    positions = special + [3, 4]
    assert _poly_device(engine, grp, eb, coeffs, positions) == capi.group_poly_eval(grp, cat(coeffs, eb), positions, threads=1)


def test_poly_eval_device_argument_checks(engine):
    q, eb = GROUPS[1]
    grp = handle(q, eb)
    d_pos = torch.tensor([1, -1, 2], dtype=torch.int64, device="cuda:0")
    out = torch.full((3 * eb,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(EngineError):
        engine.group_poly_eval_device(grp, cat([1, 2], eb), d_pos.data_ptr(), 3, out.data_ptr())      # a negative position
    with pytest.raises(EngineError):
        engine.group_poly_eval_device(grp, b"", d_pos.data_ptr(), 3, out.data_ptr())                  # t == 0
    out.fill_(0xA5)
    torch.cuda.synchronize()
    engine.group_poly_eval_device(grp, cat([1, 2], eb), d_pos.data_ptr(), 0, out.data_ptr())          # n == 0: OK, nothing written
    engine.group_poly_eval_device(grp, b"", d_pos.data_ptr(), 0, out.data_ptr())
    engine.group_dleq_responses_device(grp, out.data_ptr(), out.data_ptr(), bytes(eb), 0, out.data_ptr())
    assert engine.group_batch_scalar_mul(grp, b"", b"") == b""
    assert out.cpu().numpy().tobytes() == b"\xa5" * (3 * eb)


@functools.lru_cache(maxsize=None)
def _instance(q, n, t, seed):
    """a box of the oracle's own dealer over the group of q, with the randomness kept; computed once per shape and shared by the
    deal and extract tests, which leave it unchanged"""
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
    box = O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)
    return g, privs, pks, coeffs, ws, box


def _no_image_moduli():
    rng = random.Random(5)
    while True:
        q = H.random_odd_modulus(300, rng)
        if q % 4 == 1:
            return [5, q]


@pytest.mark.parametrize("q", _no_image_moduli(), ids=["q5", "q1mod4"])
def test_handles_without_the_constants_of_the_half_order(engine, q):
    eb = 256
    grp = ModpGroup(q)
    assert grp.has_device_scalar is False
    buf = torch.zeros(4 * eb, dtype=torch.uint8, device="cuda:0")
    d_pos = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(EngineError):
        engine.group_poly_eval_device(grp, cat([1, 2], eb), d_pos.data_ptr(), 4, buf.data_ptr())
    with pytest.raises(EngineError):
        engine.group_dleq_responses_device(grp, buf.data_ptr(), buf.data_ptr(), bytes(eb), 4, buf.data_ptr())
    with pytest.raises(EngineError):
        engine.group_batch_scalar_mul(grp, cat([1, 2], eb), cat([3, 4], eb))
    # group_deal under mode 2 takes the host path: the same bytes as mode 0, and host_calls advances
    rng = random.Random(q & 0xFFFF)
    n, t = 5, 3
    coeffs = cat([rng.randrange(q) for _ in range(t)], eb)
    pks = cat([pow(2, rng.randrange(1, q), q) or 1 for _ in range(n)], eb)
    ws = cat([rng.randrange(q) for _ in range(n)], eb)
    res = {}
    for mode in (0, 2):
        engine.set_rt_scalar(mode)
        before = engine.group_scalar_stats()
        res[mode] = engine.group_deal(grp, coeffs, list(range(1, n + 1)), pks, ws)
        after = engine.group_scalar_stats()
        assert (after["device"], after["host"]) == (before["device"], before["host"] + 1)
    assert res[0] == res[2]


DEAL_SHAPES = ((5, 3), (17, 4), (33, 2))


# q = 23 has ten admissible private keys (the units mod 22) with ten distinct public keys: the oracle's dealer serves (5, 3)
# there, but not 17 or 33 distinct keys -- those shapes run at q = 23 in test_deal_at_the_smallest_width_both_modes
DEAL_CASES = [(q, eb, n, t) for q, eb in GROUPS for n, t in DEAL_SHAPES if q != 23 or n == 5]
DEAL_IDS = [f"{q.bit_length()}b-{n}-{t}" for q, eb, n, t in DEAL_CASES]


@pytest.mark.parametrize("q,eb,n,t", DEAL_CASES, ids=DEAL_IDS)
def test_deal_mode_0_and_mode_2_against_the_oracle(engine, q, eb, n, t):
    grp = handle(q, eb)
    g, privs, pks, coeffs, ws, box = _instance(q, n, t, n * 100 + t)
    keys = [g.element_to_bytes(p) for p in pks]
    res = {}
    for mode in (0, 2):
        engine.set_rt_scalar(mode)
        before = engine.group_scalar_stats()
        res[mode] = engine.group_deal(grp, cat(coeffs, eb), list(range(1, n + 1)), cat(pks, eb), cat(ws, eb))
        after = engine.group_scalar_stats()
        want = (before["device"] + (mode == 2), before["host"] + (mode == 0))
        assert (after["device"], after["host"]) == want, (n, t, mode)
    assert res[0] == res[2], (n, t)
    r = res[2]
    assert r["X"] == cat(box["_X"], eb) and r["a1"] == cat(box["_a1"], eb) and r["a2"] == cat(box["_a2"], eb)
    assert r["Y"] == cat([box["shares"][k] for k in keys], eb)
    assert r["digest"] == box["_digest"] and r["challenge"] == box["challenge"].to_bytes(eb, "big")
    assert r["responses"] == cat([box["responses"][k] for k in keys], eb)


def test_deal_at_the_smallest_width_both_modes(engine):
    """q = 23 has too few units for the oracle's distinct keys at these n: mode 2 against mode 0 (which the protocol tests hold
    to the oracle), with unreduced coefficients and witnesses"""
    q, eb = GROUPS[0]
    grp = handle(q, eb)
    rng = random.Random(23)
    for n, t in DEAL_SHAPES:
        coeffs = cat([rng.randrange(1 << 2048) for _ in range(t)], eb)
        pks = cat([pow(2, rng.randrange(1, q), q) for _ in range(n)], eb)
        ws = cat([rng.randrange(1 << 2048) for _ in range(n)], eb)
        res = {}
        for mode in (0, 2):
            engine.set_rt_scalar(mode)
            res[mode] = engine.group_deal(grp, coeffs, list(range(1, n + 1)), pks, ws)
        assert res[0] == res[2], (n, t)


def _extract_both_modes(engine, grp, pk, y, xinv, w, n):
    res = {}
    for mode in (0, 2):
        engine.set_rt_scalar(mode)
        before = engine.group_scalar_stats()
        res[mode] = engine.group_extract_shares(grp, pk, y, xinv, w)
        after = engine.group_scalar_stats()
        want = (before["device"] + (mode == 2), before["host"] + (mode == 0))
        assert (after["device"], after["host"]) == want, (n, mode)
    assert res[0] == res[2], n
    return res[2]


@pytest.mark.parametrize("q,eb", GROUPS[1:], ids=IDS[1:])
@pytest.mark.parametrize("n,t", DEAL_SHAPES[1:])
def test_extract_mode_0_and_mode_2_against_the_oracle(engine, q, eb, n, t):
    grp = handle(q, eb)
    g, privs, pks, coeffs, ws, box = _instance(q, n, t, n * 100 + t)       # the dealt boxes of the deal test
    keys = [g.element_to_bytes(p) for p in pks]
    rng = random.Random(n)
    w2 = [H.keygen(g, rng) for _ in privs]
    base = [O.extract_secret_share(g, box, k, w) for k, w in zip(privs, w2)]
    xinv = [O.mod_inverse(k, q - 1) for k in privs]
    for zero_row in (False, True):
        if zero_row and n == 33:
            continue
        b, sbs = box, base
        if zero_row:                                               # a row with Y = 0 mod q: the non-shared branch
            b = dict(box, shares=dict(box["shares"]))
            b["shares"][keys[3]] = q
            sbs = list(base)                                       # the other rows do not depend on this one
            sbs[3] = O.extract_secret_share(g, b, privs[3], w2[3])
            assert sbs[3]["share"] == 0
        S, C = _extract_both_modes(engine, grp, cat(pks, eb), cat([b["shares"][k] for k in keys], eb), cat(xinv, eb), cat(w2, eb), n)
        assert S == cat([sb["share"] for sb in sbs], eb) and C == cat([sb["challenge"] for sb in sbs], eb)


def test_extract_at_the_smallest_width_both_modes(engine):
    """q = 23 at n = 17 and 33, where the oracle has too few distinct keys: mode 2 against mode 0 (which the protocol tests hold to
    the oracle), with unreduced xinv and w, and at n = 17 also with rows whose Y is 0 mod q (the non-shared branch)"""
    q, eb = GROUPS[0]
    grp = handle(q, eb)
    rng = random.Random(2323)
    for n in (17, 33):
        for zero_rows in ((), (3, 16)) if n == 17 else ((),):
            pk = [pow(2, rng.randrange(1, q), q) for _ in range(n)]
            y = [rng.randrange(1, q) for _ in range(n)]
            for r, v in zip(zero_rows, (0, q)):
                y[r] = v
            xinv = [rng.randrange(1 << 2048) if i % 3 else rng.randrange(q - 1) for i in range(n)]
            w = [rng.randrange(1 << 2048) if i % 2 else rng.randrange(q - 1) for i in range(n)]
            _extract_both_modes(engine, grp, cat(pk, eb), cat(y, eb), cat(xinv, eb), cat(w, eb), n)


def test_staging_is_reused_after_a_deal(engine):
    """after a mode-2 group_deal the coefficient staging of the context serves another polynomial: the new values come back"""
    q, eb = GROUPS[2]
    grp = handle(q, eb)
    g, privs, pks, coeffs, ws, box = _instance(q, 5, 3, seed=77)
    engine.set_rt_scalar(2)
    engine.group_deal(grp, cat(coeffs, eb), list(range(1, 6)), cat(pks, eb), cat(ws, eb))
    rng = random.Random(78)
    for t in (2, 5):
        other = [rng.randrange(1 << 2048) for _ in range(t)]
        positions = list(range(1, 18))
        assert _poly_device(engine, grp, eb, other, positions) == capi.group_poly_eval(grp, cat(other, eb), positions, threads=1)
