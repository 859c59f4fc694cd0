"""Forward differences for X_i of a run-time MODP group on the GPU (k_rt_commit_eval_mont, k_rt_fd_chain, k_rt_from_mont
behind mpvss_modp_group_commit_eval, _verify_distribution and _distribute).

A context of this module's own runs every call in mode 2 (forward differences whenever admissible) and again in mode 0
(Horner's rule); the two results are compared byte for byte, and against Python integers (Horner's rule in the exponent,
which is prod_j C_j^(i^j) as an integer identity).  mpvss_modp_group_fd_stats tells which path a call took."""
import ctypes as C
import random

import pytest
import torch

import mpvss_oracle as O
import modp_rt_helpers as H
from mpvss_rs_amd import Engine, ModpGroup, capi

pytestmark = pytest.mark.gpu

E_INVALID = -1
MPVSS_HOST, MPVSS_DEVICE = capi.MPVSS_HOST, capi.MPVSS_DEVICE


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _q(bits):
    if bits == 3072:
        return _q3072()
    return H.rfc_prime(bits) if bits in H.RFC_C else H.small_safe_primes()[bits]


_Q3072 = []


def _q3072():
    """an odd 3072-bit modulus (the identities hold for any odd q; the commitments below are units of it)"""
    if not _Q3072:
        _Q3072.append(H.random_odd_modulus(3072, random.Random(3072)))
    return _Q3072[0]


_GROUPS = {}


def _group(bits):
    if bits not in _GROUPS:
        _GROUPS[bits] = ModpGroup(_q(bits), elem_bytes=384) if bits == 3072 else ModpGroup(_q(bits))
    return _GROUPS[bits]


def enc(v, EB):
    return v.to_bytes(EB, "big")


def cat(vals, EB):
    return b"".join(enc(v, EB) for v in vals)


def split(b, EB):
    return [int.from_bytes(b[i:i + EB], "big") for i in range(0, len(b), EB)]


def horner_int(Cs, q, i):
    acc = Cs[-1] % q
    for c in reversed(Cs[:-1]):
        acc = pow(acc, i, q) * c % q
    return acc


def units(t, q, rng):
    """t commitments that are units mod q"""
    import math
    out = []
    while len(out) < t:
        c = rng.randrange(2, q)
        if math.gcd(c, q) == 1:
            out.append(c)
    return out


def commit_eval(e, grp, cbytes, positions, space=MPVSS_HOST):
    if space == MPVSS_HOST:
        return e.group_commit_eval(grp, cbytes, positions)
    EB, n = grp.elem_bytes, len(positions)
    d_c = torch.frombuffer(bytearray(cbytes), dtype=torch.uint8).cuda()
    d_p = torch.tensor(positions, dtype=torch.int64).cuda()
    d_o = torch.zeros(n * EB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = e.lib.mpvss_modp_group_commit_eval(e.ctx, grp.handle, MPVSS_DEVICE, C.c_void_p(d_c.data_ptr()), len(cbytes) // EB,
                                            C.c_void_p(d_p.data_ptr()), n, C.c_void_p(d_o.data_ptr()))
    assert rc == 0, rc
    return bytes(d_o.cpu().numpy())


def both_modes(e, call, mode=2, chains=0):
    """call() under `mode` and under mode 0: (result, path taken under `mode`, result of mode 0)"""
    e.set_rt_fd(mode, chains)
    s0 = e.group_fd_stats()
    got = call()
    s1 = e.group_fd_stats()
    e.set_rt_fd(0, 0)
    ref = call()
    s2 = e.group_fd_stats()
    e.set_rt_fd(2, 0)
    assert s2["fd"] == s1["fd"] and s2["horner"] > s1["horner"], "mode 0 did not take Horner's rule"
    path = "fd" if s1["fd"] > s0["fd"] else "horner"
    assert (s1["fd"] - s0["fd"] > 0) != (s1["horner"] - s0["horner"] > 0), (s0, s1)
    return got, path, ref


def check_x(grp, Cs, positions, got, sample=None):
    EB, q = grp.elem_bytes, grp.q
    vals = split(got, EB)
    assert len(vals) == len(positions)
    idx = range(len(positions)) if sample is None else sample
    for k in idx:
        assert vals[k] == horner_int(Cs, q, positions[k]), (k, positions[k])


T_LIST = (2, 3, 15, 16, 17, 33, 64)
P0S = (0, 1, 1000, 2 ** 40)


@pytest.mark.parametrize("bits", [40, 256, 1024, 2048, 3072])
def test_parity_fd_against_horner_and_python(eng, bits):
    grp = _group(bits)
    q, EB = grp.q, grp.elem_bytes
    rng = random.Random(bits)
    for ti, t in enumerate(T_LIST):
        Cs = units(t, q, rng)
        given = list(Cs)
        if q + Cs[1] < 1 << (8 * EB):
            given[1] = Cs[1] + q                      # a commitment >= q: reduced, forward differences still taken
        cb = cat(given, EB)
        for ni, (n, chains) in enumerate(((t, 1), (t + 1, 1), (2 * t + 5, 2), (4 * t + 3, 3))):
            p0 = P0S[(ni + ti) % 4]
            if p0 + n - 1 >= q - 1:
                p0 = 1000                             # the 40-bit prime: 2^40 is past q - 1
            positions = list(range(p0, p0 + n))
            space = MPVSS_DEVICE if (ni + ti) % 2 else MPVSS_HOST
            got, path, ref = both_modes(eng, lambda: commit_eval(eng, grp, cb, positions, space), chains=chains)
            assert path == "fd", (bits, t, n, chains, p0)
            assert got == ref, (bits, t, n, chains, p0)
            sample = None if t <= 17 else sorted({0, 1, n // 2 - 1, n // 2, n - 2, n - 1})
            check_x(grp, Cs, positions, got, sample)


def test_chains_setting_is_clamped_and_automatic(eng):
    grp = _group(256)
    rng = random.Random(5)
    t, n = 5, 57
    Cs = units(t, grp.q, rng)
    cb = cat(Cs, grp.elem_bytes)
    positions = list(range(7, 7 + n))
    outs = []
    for chains in (0, 1, 2, 3, 11, 12, 1000):          # 57 // 5 = 11 chains at the most
        got, path, ref = both_modes(eng, lambda: commit_eval(eng, grp, cb, positions), chains=chains)
        assert path == "fd" and got == ref, chains
        outs.append(got)
    check_x(grp, Cs, positions, outs[0])
    assert all(o == outs[0] for o in outs)


def test_largest_t_at_1024_bits(eng):
    grp = _group(1024)
    t = grp.fd_max_t
    assert t >= 256
    rng = random.Random(1024)
    Cs = units(t, grp.q, rng)
    cb = cat(Cs, grp.elem_bytes)
    n = 4 * t + 3
    positions = list(range(1, 1 + n))
    got, path, ref = both_modes(eng, lambda: commit_eval(eng, grp, cb, positions), chains=3)
    assert path == "fd" and got == ref
    check_x(grp, Cs, positions, got, sorted({0, 1, t - 1, t, n // 2, n - 2, n - 1}))
    # one past it: Horner's rule, the same bytes as mode 0
    Cs.append(3)
    cb = cat(Cs, grp.elem_bytes)
    got, path, ref = both_modes(eng, lambda: commit_eval(eng, grp, cb, positions[: t + 9]))
    assert path == "horner" and got == ref


def test_floors_of_t_max():
    assert all(_group(b).fd_max_t >= 256 for b in (40, 256, 1024, 2048))
    assert _group(3072).fd_max_t >= 128


@pytest.mark.parametrize("space", [MPVSS_HOST, MPVSS_DEVICE], ids=["host", "device"])
def test_inadmissible_calls_take_horner(eng, space):
    grp = _group(256)
    q, EB = grp.q, grp.elem_bytes
    rng = random.Random(9)
    Cs = units(4, q, rng)
    run = lambda cs, pos, **kw: both_modes(eng, lambda: commit_eval(eng, grp, cat(cs, EB), pos, space), **kw)
    consecutive = list(range(3, 23))
    got, path, ref = run(Cs, consecutive)
    assert path == "fd" and got == ref                                         # the admissible call, for contrast
    cases = {
        "t = 1": (Cs[:1], consecutive),
        "gap": (Cs, [3, 4, 6] + list(range(7, 24))),
        "descending": (Cs, consecutive[::-1]),
        "commitment 0": (Cs[:2] + [0] + Cs[3:], consecutive),
        "commitment q": (Cs[:2] + [q] + Cs[3:], consecutive),
        "fewer positions than seeds": (Cs, [5, 6, 7]),
    }
    for name, (cs, pos) in cases.items():
        got, path, ref = run(cs, pos)
        assert path == "horner", name
        assert got == ref, name
        assert split(got, EB) == [_reference(cs, q, i) for i in pos], name
    # mode 1 below fd_min_shares
    assert grp.fd_min_shares(4) > len(consecutive)
    got, path, ref = run(Cs, consecutive, mode=1)
    assert path == "horner" and got == ref


def _reference(cs, q, i):
    """prod_j C_j^(i^j mod (q-1)) as the reference forms it (k_rt_commit_eval's contract, a commitment that is 0 mod q included)"""
    x = 1
    for j, c in enumerate(cs):
        x = x * pow(c % q, (i ** j) % (q - 1), q) % q
    return x


def test_positions_reaching_q_minus_1_take_horner(eng):
    grp = _group(40)
    q, EB = grp.q, grp.elem_bytes
    Cs = units(3, q, random.Random(40))
    cb = cat(Cs, EB)
    pos = list(range(q - 4, q + 4))                      # n = 8 around q - 1, where Horner reduces the position
    got, path, ref = both_modes(eng, lambda: commit_eval(eng, grp, cb, pos))
    assert path == "horner" and got == ref
    assert split(got, EB) == [horner_int(Cs, q, i % (q - 1)) for i in pos]
    pos = list(range(q - 9, q - 1))                      # the last admissible run: up to q - 2
    got, path, ref = both_modes(eng, lambda: commit_eval(eng, grp, cb, pos))
    assert path == "fd" and got == ref
    check_x(grp, Cs, pos, got)


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
    coeffs = [rng.randrange(1, g.q - 1) for _ in range(t)]
    ws = [H.keygen(g, rng) for _ in range(n)]
    return g, pks, coeffs, ws, O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)


@pytest.mark.parametrize("bits", [1024, 2048])
def test_protocol_verify_and_distribute(eng, bits):
    grp = _group(bits)
    EB = grp.elem_bytes
    n, t = 40, 17
    g, pks, coeffs, ws, box = _instance(grp.q, n, t, bits)
    flat = O.box_to_flat(g, box)
    keys = [g.element_to_bytes(p) for p in pks]
    positions = list(range(1, n + 1))
    Y = cat([box["shares"][k] for k in keys], EB)
    R = cat([box["responses"][k] for k in keys], EB)
    ch = enc(box["challenge"], EB)
    verify = lambda shares: eng.group_verify_distribution(grp, flat["commitments"], positions, cat(pks, EB), shares, R, ch, dump=True)
    v, path, v0 = both_modes(eng, lambda: verify(Y))
    assert path == "fd"
    assert v["verdict"] is True and v["digest"] == box["_digest"]
    assert v == v0
    assert split(v["X"], EB) == box["_X"]
    bad = bytearray(Y)
    bad[7 * EB + EB - 1] ^= 1                                                   # one tampered share
    v, path, v0 = both_modes(eng, lambda: verify(bytes(bad)))
    assert path == "fd" and v["verdict"] is False and v0["verdict"] is False and v == v0
    P = [O.poly_get_value(coeffs, i) % (g.q - 1) for i in positions]
    d, path, d0 = both_modes(eng, lambda: eng.group_distribute(grp, flat["commitments"], positions, cat(pks, EB), cat(P, EB), cat(ws, EB)))
    assert path == "fd" and d == d0
    assert split(d["X"], EB) == box["_X"] and d["digest"] == box["_digest"]


def test_error_contract(eng):
    lib, grp = eng.lib, _group(256)
    assert lib.mpvss_ctx_set_rt_fd(None, 1, 0) == E_INVALID
    for mode, chains in ((-1, 0), (3, 0), (1, -1)):
        assert lib.mpvss_ctx_set_rt_fd(eng.ctx, mode, chains) == E_INVALID
    assert lib.mpvss_modp_group_fd_min_shares(None, 4) == E_INVALID
    assert lib.mpvss_modp_group_fd_min_shares(grp.handle, 0) == E_INVALID
    assert lib.mpvss_modp_group_fd_max_t(None) == E_INVALID
    assert lib.mpvss_modp_group_fd_stats(None, None, None) == E_INVALID
    assert lib.mpvss_modp_group_fd_stats(eng.ctx, None, None) == 0
    assert grp.fd_min_shares(4) >= 1
    eng.set_rt_fd(2, 0)
